"""Output-rate conversion (pe_set_output_rate, kernels/resample.h) on the test-only emulator build of the engine: the kernel
against the f64 restatement of the filter in tests/resample_case.py (noise rows, tones, indices past 2^31 / M), whole
utterances and the three kinds of streams at 8000 and 48000 Hz on poisoned workspaces, the native-rate engine untouched,
and the errors. The GPU counterpart is tests/test_gpu_resample.py (-m gpu)."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import resample_case as R                                # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402

PAIRS = [(16000, 8000), (16000, 22050), (16000, 48000), (22050, 8000), (22050, 48000)]
CHUNK, FIRST = 4, 2


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _engine(lib, fs_in=16000, preset="tiny", device=0):
    cfg = W.preset(preset)
    if fs_in != cfg.sample_rate:
        cfg = dataclasses.replace(cfg, sample_rate=fs_in)
    w = W.synthetic_weights(cfg, 1234)
    return cfg, w, Engine(blob=W.pack_blob(cfg, w), lib=lib, device=device)


# ---- 1. pointwise, 3. large indices, 2. tones: the kernel alone, through pe_debug_resample
def noise_rows(eng, fs_in, fs_out):
    rng = np.random.default_rng(fs_in + fs_out)
    rows = [rng.standard_normal(n).astype(np.float32) for n in (1, 37, 1024, 1500)]
    got = eng.debug_resample(rows)
    for x, y in zip(rows, got):
        assert y.size == R.n_out(x.size, fs_in, fs_out)
        want, bound = R.truth(x, fs_in, fs_out)
        R.assert_within(y, want, bound, f"{fs_in}->{fs_out}, noise row of {x.size}")


def large_indices(eng):
    fs_in, fs_out, n0 = 22050, 48000, 33_000_000
    p = R.params(fs_in, fs_out)
    assert n0 * p.M > 2 ** 32
    origin = n0 * p.M // p.L - p.K - 3                    # the row starts a little before the first tap
    x = np.random.default_rng(5).standard_normal(256 * p.M // p.L + 2 * p.K + 8).astype(np.float32)
    got = eng.debug_resample([x], n0=[n0], count=[256], origin=[origin])[0]
    want, bound = R.truth(x, fs_in, fs_out, n0=n0, count=256, origin=origin)
    assert np.max(np.abs(want)) > 0.1
    R.assert_within(got, want, bound, f"{fs_in}->{fs_out}, outputs from {n0}")


def tones(eng, fs_in, fs_out):
    p = R.params(fs_in, fs_out)
    skip = int(p.K * fs_out / fs_in) + 2
    j = np.arange(6000, dtype=np.float64)
    for rel in (0.1, 0.5, 0.8):
        f = rel * p.fmin / 2
        x = np.cos(2 * np.pi * f * j / fs_in).astype(np.float32)
        got = eng.debug_resample([x])[0]
        gain, res = R.tone_figures(got, f, fs_out, skip)
        tgain, tres = R.tone_figures(R.truth(x, fs_in, fs_out)[0], f, fs_out, skip)
        print(f"{fs_in}->{fs_out} tone at {rel} of fmin/2: gain {gain:+.4f} dB (f64 {tgain:+.4f}), rest {res:.1f} dB (f64 {tres:.1f})")
        assert abs(gain) <= 0.1 and res <= -85.0, (fs_in, fs_out, rel, gain, res)
    if fs_out < fs_in:
        f = 1.1 * fs_out / 2
        x = np.cos(2 * np.pi * f * j / fs_in).astype(np.float32)
        lev = R.level_db(eng.debug_resample([x])[0], skip)
        tlev = R.level_db(R.truth(x, fs_in, fs_out)[0], skip)
        print(f"{fs_in}->{fs_out} tone at 1.1 x output Nyquist comes out at {lev:.1f} dB (f64 {tlev:.1f})")
        assert lev <= -100.0, (fs_in, fs_out, lev)


@pytest.mark.parametrize("fs_in", [16000, 22050])
def test_kernel_against_f64_truth(emu_lib, fs_in):
    """Noise rows of 1, 37, 1024 and 1500 samples in one batch (ragged, shorter than K, across a tile), tones in and just
    above the pass band, and -- at 22050 -> 48000 -- outputs from index 33 000 000 on, where n x M needs 64 bits."""
    _, _, eng = _engine(emu_lib, fs_in)
    for a, b in PAIRS:
        if a != fs_in:
            continue
        eng.set_output_rate(b)
        p = R.params(a, b)
        assert (eng.native_rate, eng.output_rate, eng.resample_half_width) == (a, b, p.K)
        assert p.K == {(16000, 8000): 35, (22050, 8000): 48}.get((a, b), 18)
        noise_rows(eng, a, b)
        tones(eng, a, b)
    if fs_in == 22050:
        eng.set_output_rate(48000)
        large_indices(eng)
    eng.close()


# ---- 4. whole utterances
def whole_utterances(eng, cfg, rate, native, durations):
    from oracle import vits_oracle as O
    ids, nw, nz = K.inputs(cfg)
    fs_in, hop = cfg.sample_rate, eng.hop
    eng.set_output_rate(rate)
    r = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    assert np.array_equal(r.frames, native.frames) and np.array_equal(eng.durations(), durations)
    for b in range(len(ids)):
        x = eng.debug_tensor("audio", b)[0]
        assert x.size == int(r.frames[b]) * hop
        assert r.audio[b].size == r.pcm[b].size == R.n_out(x.size, fs_in, rate)      # offsets = prefix sums of N_out
        want, bound = R.truth(x, fs_in, rate)
        R.assert_within(r.audio[b], want, bound, f"{fs_in}->{rate}, utterance {b} of {int(r.frames[b])} frames")
        assert np.array_equal(O.audio_float_to_int16(r.audio[b]), r.pcm[b]), b
    return r


def test_whole_utterances(emu_lib, monkeypatch):
    """The three ragged texts as one batch at 8000 and 48000 Hz on poisoned workspaces: every utterance is the f64 resampling
    of the native waveform of the same call, its int16 the conversion of ITS floats, lengths ceil(S L / M); frames and
    durations are the native call's."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, _, eng = _engine(emu_lib)
    ids, nw, nz = K.inputs(cfg)
    native = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    durations = eng.durations()
    assert len(set(int(f) for f in native.frames)) == 3
    for rate in (8000, 48000):
        whole_utterances(eng, cfg, rate, native, durations)
    eng.close()


# ---- 5. streams
def one_streams(eng, cfg, rate):
    from oracle import vits_oracle as O
    texts = P.emu_texts(cfg, False)[:3]
    eng.set_output_rate(0)
    nat = [P.one_stream(eng, x, [FIRST, CHUNK]) for x in texts]
    eng.set_output_rate(rate)
    for x, (nchunks, frames) in zip(texts, nat):
        got, f2 = P.one_stream(eng, x, [FIRST, CHUNK])
        sizes = P.expected_sizes(frames, FIRST, CHUNK)
        assert f2 == frames and len(got) == len(nchunks) == len(sizes)
        R.check_chunks(got, sizes, [a for a, _ in nchunks], eng.hop, cfg.sample_rate, rate, O,
                       f"{cfg.sample_rate}->{rate}, one-utterance stream of {x.name}")


def lock_step(eng, cfg, rate):
    from oracle import vits_oracle as O
    ids, nw, nz = K.inputs(cfg)
    sizes_of = lambda k: FIRST if k == 0 else CHUNK      # noqa: E731
    eng.set_output_rate(0)
    nat, _ = K.drain(eng, ids, nw, nz, chunk_frames=sizes_of)
    frames = [int(f) for f in eng.stream_frames]
    eng.set_output_rate(rate)
    got, _ = K.drain(eng, ids, nw, nz, chunk_frames=sizes_of)
    assert [int(f) for f in eng.stream_frames] == frames
    for b in range(len(ids)):
        sizes = P.expected_sizes(frames[b], FIRST, CHUNK)
        assert len(got[b]) == len(nat[b]) == len(sizes)
        R.check_chunks(got[b], sizes, [a for a, _ in nat[b]], eng.hop, cfg.sample_rate, rate, O,
                       f"{cfg.sample_rate}->{rate}, lock-step stream, utterance {b}")


def pool(eng, cfg, rate, multi_speaker=False):
    from oracle import vits_oracle as O
    eng.set_output_rate(0)
    nat = P.emu_texts(cfg, multi_speaker)
    halo0 = R.play_pool(eng, nat, CHUNK, FIRST)
    eng.set_output_rate(rate)
    got = P.emu_texts(cfg, multi_speaker)
    halo = R.play_pool(eng, got, CHUNK, FIRST)
    assert halo == halo0 + 1                             # one more exact frame on each side of a window
    assert sum(1 for x in got if x.left) == 1
    for x, n in zip(got, nat):
        assert x.sizes == n.sizes and x.frames == n.frames and x.left == n.left, x.name
        R.check_chunks(x.chunks, x.sizes, [a for a, _ in n.chunks], eng.hop, cfg.sample_rate, rate, O,
                       f"{cfg.sample_rate}->{rate}, pool listener {x.name}", cut=x.left)


@pytest.mark.parametrize("rate", [8000, 48000])
def test_streams(emu_lib, monkeypatch, rate):
    """The one-utterance stream, the lock-step stream and the pool scenario, chunks of 4 frames and first chunks of 2: every
    chunk has ceil(s1 L / M) - ceil(s0 L / M) samples, an utterance's chunks are the f64 resampling of the native chunks of an
    identical native-rate run on the same injected noise, every chunk's int16 is the conversion of its floats."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, _, eng = _engine(emu_lib)
    one_streams(eng, cfg, rate)
    lock_step(eng, cfg, rate)
    pool(eng, cfg, rate)
    eng.close()


# ---- 6. nothing else moved
def nothing_else_moved(make_engine, graphs):
    """Two engines make the same calls -- a batch on injected noise, then one utterance on the engine's own noise (the
    speculative one-graph form on the GPU) -- twice over; one of them delivers the first round at 48000 Hz. Equal seeds
    and run counters give both the same draws."""
    cfg, _, eng = make_engine()
    _, _, fresh = make_engine()
    ids, nw, nz = K.inputs(cfg)
    one, sc = ids[0], (0.667, 0.5, 0.8)                  # a handful of frames: always the smallest frame bucket

    def calls(e):
        a = e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        la = e.run_launches
        b = e.synthesize(one, sc)
        return a, la, b, e.run_launches

    f1 = calls(fresh)
    f2 = calls(fresh)
    eng.set_output_rate(48000)
    r1 = calls(eng)
    eng.set_output_rate(eng.native_rate)
    assert eng.output_rate == cfg.sample_rate and eng.resample_half_width == 0
    n2 = calls(eng)
    assert (n2[1], n2[3]) == (f2[1], f2[3]), (n2[1], n2[3], f2[1], f2[3])
    for got, want in ((n2[0], f2[0]), (n2[2], f2[2])):
        assert np.array_equal(got.frames, want.frames)
        for x, y in zip(got.audio + got.pcm, want.audio + want.pcm):
            assert x.size and np.array_equal(x, y)
    assert np.array_equal(r1[0].frames, f1[0].frames) and np.array_equal(r1[2].frames, f1[2].frames)
    assert r1[2].pcm[0].size == R.n_out(int(f1[2].frames[0]) * eng.hop, cfg.sample_rate, 48000)
    print(f"launches: batch {f1[1]} native / {r1[1]} at 48000, one utterance {f1[3]} / {r1[3]}")
    assert r1[1] <= f1[1] + 2 and r1[3] <= f1[3] + 2, (r1[1], f1[1], r1[3], f1[3])
    eng.set_output_rate(8000)
    for _ in range(3):
        eng.synthesize(one, sc)
    c0 = eng.graph_stats[1]
    for _ in range(4):
        eng.synthesize(one, sc)
    assert eng.graph_stats[1] == c0, (c0, eng.graph_stats)
    assert not graphs or c0 > 0
    eng.close()
    fresh.close()


def test_native_rate_is_untouched(emu_lib):
    """Set 48000, synthesise, set the native rate again, synthesise: audio, pcm, frames and the launch counts are those of
    an engine that never had a rate set, bit for bit; a rate costs at most two launches per call; captures stop growing."""
    nothing_else_moved(lambda: _engine(emu_lib), graphs=False)


# ---- 7. errors
def test_errors(emu_lib):
    """Every refused setting names what is wrong and leaves the engine working at its previous setting."""
    cfg, _, eng = _engine(emu_lib)
    ids, nw, nz = K.inputs(cfg)
    eng.set_output_rate(8000)
    before = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])

    def same():
        assert (eng.native_rate, eng.output_rate) == (16000, 8000)
        r = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
        assert np.array_equal(r.audio[0], before.audio[0]) and np.array_equal(r.pcm[0], before.pcm[0])

    for bad in (7999, 48001):
        with pytest.raises(EngineError, match=rf"16000 -> {bad}"):
            eng.set_output_rate(bad)
        same()
    with pytest.raises(EngineError, match=r"16000 -> 44099.*640"):
        eng.set_output_rate(44099)
    same()
    with pytest.raises(EngineError, match=r"22050 contradicts.*16000"):
        eng.set_output_rate(48000, native=22050)
    same()
    with eng.stream_pool(2, 48):
        with pytest.raises(EngineError, match="stream pool is open"):
            eng.set_output_rate(48000)
        with pytest.raises(EngineError, match="stream pool is open"):
            eng.set_output_rate(0)
    same()
    eng.close()
    # an .onnx carries no rate: 0 has nothing to stand for, the caller's value is taken
    onnx = Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), lib=emu_lib)
    assert onnx.sample_rate == 0
    with pytest.raises(EngineError, match="carries none"):
        onnx.set_output_rate(8000)
    with pytest.raises(EngineError, match="no output rate set"):
        onnx.debug_resample([np.zeros(8, np.float32)])
    onnx.set_output_rate(8000, native=16000)
    assert (onnx.native_rate, onnx.output_rate, onnx.resample_half_width) == (16000, 8000, 35)
    y = onnx.debug_resample([np.ones(64, np.float32)])[0]
    assert y.size == 32 and abs(float(y[16]) - 1.0) < 0.05
    onnx.close()


def test_infer_output_rate(emu_lib, tmp_path):
    """python -m piper_amd.infer --output-rate: the WAV says the output rate and holds ceil(S L / M) samples of the same
    utterance the native run writes."""
    import io
    import json
    import wave
    from piper_amd import infer
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    line = json.dumps({"phoneme_ids": [int(v) for v in W.synthetic_phoneme_ids(9, 3, id_max=39)]}) + "\n"
    sizes = {}
    for name, extra in (("native", []), ("out", ["--output-rate", "8000"])):
        d = tmp_path / name
        args = ["--model", model, "--output-dir", str(d), "--sample-rate", "16000", "--seed", "5", "--noise-scale", "0",
                "--noise-scale-w", "0"] + extra
        assert infer.main(args, stdin=io.StringIO(line), lib=emu_lib) == 0
        with wave.open(str(d / "0.wav"), "rb") as w:
            sizes[name] = (w.getframerate(), w.getnframes())
    assert sizes["native"][0] == 16000 and sizes["out"][0] == 8000
    assert sizes["out"][1] == R.n_out(sizes["native"][1], 16000, 8000) and sizes["out"][1] > 0


# ---- a missed speculative guess: the second half runs again on a workspace that moved
def missed_guess(eng, cfg, rate):
    """One-utterance calls on the engine's own prior noise (the speculative form): after two calls at length scale 1 a call
    at 6 overruns the guessed frame bucket and the workspace, so the second half is issued again on buffers that were
    re-allocated in between. Every call, the missed one included, is checked like the whole utterances above."""
    from oracle import vits_oracle as O
    eng.set_output_rate(rate)
    rng = np.random.default_rng(93)
    for it, ls in enumerate((1.0, 1.0, 6.0, 1.0)):      # ~34 frames, then ~200: past the 128 the workspace holds
        ids = W.synthetic_phoneme_ids(20, it, id_max=cfg.n_vocab - 1)
        nw = rng.standard_normal((2, 20)).astype(np.float32)
        r = eng.synthesize(ids, (0.0, ls, 0.8), noise_w=nw)
        x = eng.debug_tensor("audio", 0)[0]
        assert x.size == int(r.frames[0]) * eng.hop and np.max(np.abs(x)) > 1e-3
        fs_out = rate or cfg.sample_rate
        assert r.audio[0].size == r.pcm[0].size == R.n_out(x.size, cfg.sample_rate, fs_out), it
        if rate:
            want, bound = R.truth(x, cfg.sample_rate, rate)
            R.assert_within(r.audio[0], want, bound, f"{cfg.sample_rate}->{rate}, call {it} at length scale {ls}")
        else:
            assert np.array_equal(r.audio[0], x), it
        assert np.array_equal(O.audio_float_to_int16(r.audio[0]), r.pcm[0]), it
    runs, misses = eng.speculation_stats
    print(f"rate {rate}: {runs} speculative runs, {misses} missed")
    assert runs >= 2 and misses >= 1, (runs, misses)


@pytest.mark.parametrize("rate", [0, 48000])
def test_missed_guess(emu_lib, rate):
    cfg, _, eng = _engine(emu_lib)
    missed_guess(eng, cfg, rate)
    eng.close()
