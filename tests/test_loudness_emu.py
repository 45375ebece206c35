"""Target loudness (pe_set_loudness, kernels/loudness.h) on the test-only emulator build of the engine: the filter table, the
two kernels against the f64 restatement of tests/loudness_case.py, whole utterances at the native rate and at 8000 / 48000 Hz
on poisoned workspaces, the speculative one-utterance form, the untouched default, the untouched streams, the command-line
tool and the refusals. The GPU counterpart is tests/test_gpu_loudness.py (-m gpu)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError, Timing, loudness_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import loudness_case as LC                               # noqa: E402
import resample_case as R                                # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402

CHUNK, FIRST = 4, 2
TARGET, CEILING = -23.0, -1.0
STRETCH = 60            # frames of the third utterance: 15360 samples = 9.6 segments of 100 ms at any rate, six blocks
NAMES = ("loudness_seg_kernel", "loudness_gain_kernel", "pcm16_gain_kernel")


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _engine(lib, preset="tiny", device=0):
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, 1234)
    return cfg, w, Engine(blob=W.pack_blob(cfg, w), lib=lib, device=device)


# ---- 1. coefficients
def test_coefficients(emu_lib):
    """pe_loudness_filter(48000) is the table of ITU-R BS.1770-4 to 1e-12, and the f64 restatement at every rate."""
    c = loudness_filter(48000, emu_lib)
    t = LC.TABLE_48K
    want = list(t["shelf_b"]) + list(t["shelf_a"]) + [1.0, -2.0, 1.0] + list(t["hp_a"])
    assert np.max(np.abs(c - np.asarray(want))) <= 1e-12, c - np.asarray(want)
    for fs in LC.RATES:
        assert np.max(np.abs(loudness_filter(fs, emu_lib) - np.asarray(LC.coefficients(fs)))) <= 1e-14, fs
    with pytest.raises(EngineError, match="3999"):
        loudness_filter(3999, emu_lib)


# ---- 2. the kernels alone
@pytest.mark.parametrize("fs", LC.RATES)
def test_kernel_against_f64_truth(emu_lib, fs):
    """One ragged batch per rate: the bursts at lengths 0, 1, h - 1, 4h - 1, 4h, 4h + 1, 5h - 1, 5h, 13h + 7 (both gates drop
    blocks of the longest), a row with a DC offset, an all-zero row and, at 48000 Hz, the calibration sine: L within 1e-3 LU,
    scale within 2e-4, flags equal, two runs bit-equal."""
    _, _, eng = _engine(emu_lib)
    LC.check_kernel(eng, fs)
    eng.close()


# ---- 3. whole utterances
def whole_utterances(eng, cfg, rate):
    """The three ragged texts, the third stretched to STRETCH frames by a timing plan, with the setting off and on: equal
    floats, the report against the f64 loudness of those floats, the int16 the conversion with the reported scale; at
    T = -5 every measurable utterance is LIMITED and stays under the ceiling."""
    from oracle import vits_oracle as O
    ids, nw, nz = K.inputs(cfg)
    nz = np.ascontiguousarray(np.pad(nz, ((0, 0), (0, 0), (0, max(0, STRETCH + 8 - nz.shape[2])))))
    plan = Timing(target_frames=[0, 0, STRETCH])
    eng.set_output_rate(rate or 0)
    fs = rate or cfg.sample_rate
    eng.set_loudness(None)
    off = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
    assert eng.last_loudness()[0].size == 0
    assert int(off.frames[2]) == STRETCH and len(set(int(f) for f in off.frames)) == 3
    for a, p in zip(off.audio, off.pcm):
        assert np.array_equal(O.audio_float_to_int16(a), p)
    for target in (TARGET, -5.0):
        eng.set_loudness(target, CEILING)
        assert eng.loudness() == (target, CEILING)
        on = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
        assert np.array_equal(on.frames, off.frames)
        for a, b in zip(on.audio, off.audio):
            assert a.size and np.array_equal(a.view(np.int32), b.view(np.int32))
        _, _, _, flags = LC.check_delivery(eng, on, fs, target, CEILING, f"rate {fs}, T {target}: ")
        assert not flags[2] & LC.SHORT
        if target == -5.0:
            assert all(f & (LC.LIMITED | LC.UNMEASURABLE) for f in flags), flags
    eng.set_loudness(None)


@pytest.mark.parametrize("rate", [0, 8000, 48000])
def test_whole_utterances(emu_lib, monkeypatch, rate):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, _, eng = _engine(emu_lib)
    whole_utterances(eng, cfg, rate)
    eng.close()


def test_whole_utterances_f16x3(emu_lib, monkeypatch):
    """The same under PIPER_HIP_MATRIX=f16x3 (read at engine creation), whose generator tail is another kernel."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    monkeypatch.setenv("PIPER_HIP_MATRIX", "f16x3")
    cfg, _, eng = _engine(emu_lib)
    whole_utterances(eng, cfg, 0)
    eng.close()


# ---- 4. the speculative one-utterance form
def speculative(make_engine, graphs):
    """Two engines with equal seeds make the same calls with the setting on, one through synthesize, one through
    synthesize_batch of one utterance: after the warm-up every call is the one-graph form with a constant launch count, new
    T / C values capture nothing, both engines deliver the same bits; then a call whose guess misses still delivers the
    conversion of its own floats at its own loudness."""
    cfg, _, a = make_engine()
    _, _, b = make_engine()
    one, sc = W.synthetic_phoneme_ids(20, 3, id_max=cfg.n_vocab - 1), (0.667, 1.0, 0.8)
    fs = cfg.sample_rate
    for e in (a, b):
        e.set_loudness(TARGET, CEILING)
        if graphs:
            e.warmup(1, 32, sample_ids=one)
        else:                                            # (the emulator captures nothing: one call gives the estimate)
            e.synthesize(one, sc)
    runs0 = a.speculation_stats[0]
    got, launches = [], []
    for k in range(3):
        got.append(a.synthesize(one, sc))
        launches.append(a.run_launches)
        LC.check_delivery(a, got[-1], fs, TARGET, CEILING, f"speculative call {k}: ")
        rb = b.synthesize_batch([one], sc)
        assert np.array_equal(got[-1].audio[0], rb.audio[0]) and np.array_equal(got[-1].pcm[0], rb.pcm[0]), k
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a.last_loudness(), b.last_loudness()))
    assert a.speculation_stats[0] == runs0 + 3 and len(set(launches)) == 1, (a.speculation_stats, launches)
    c0 = a.graph_stats[1]
    assert not graphs or c0 > 0
    for target, ceil in ((-16.0, -3.0), (-30.0, 0.0)):
        a.set_loudness(target, ceil)
        r = a.synthesize(one, sc)
        assert a.run_launches == launches[0]
        LC.check_delivery(a, r, fs, target, ceil, f"T {target}, ceiling {ceil}: ")
    assert a.graph_stats[1] == c0 and a.speculation_stats[0] == runs0 + 5, (c0, a.graph_stats, a.speculation_stats)
    # a longer text at a slow rate after the short ones: the guess misses, the second half runs again
    m0 = a.speculation_stats[1]
    rng = np.random.default_rng(93)
    r = a.synthesize(W.synthetic_phoneme_ids(20, 5, id_max=cfg.n_vocab - 1), (0.0, 6.0, 0.8),
                     noise_w=rng.standard_normal((2, 20)).astype(np.float32))
    assert a.speculation_stats[1] == m0 + 1, a.speculation_stats
    LC.check_delivery(a, r, fs, -30.0, 0.0, "missed guess: ")
    a.close()
    b.close()


def test_speculative_form(emu_lib):
    speculative(lambda: _engine(emu_lib), graphs=False)


# ---- 5. off is the parent
def off_is_parent(make_engine):
    """An engine that never had the setting and one that had it set and cleared make the same calls: equal bits, the
    reference's rule, equal launch counts, and no loudness kernel among the launches (the profile's per-kernel rows; the
    same rows do name them while the setting is on)."""
    from oracle import vits_oracle as O
    cfg, _, fresh = make_engine()
    _, _, eng = make_engine()
    ids, nw, nz = K.inputs(cfg)
    one, sc = ids[0], (0.667, 0.5, 0.8)

    def calls(e):
        x = e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        lx = e.run_launches
        y = e.synthesize(one, sc)
        return x, lx, y, e.run_launches

    eng.set_loudness(-16.0, -2.0)
    on = calls(eng)
    eng.set_loudness(None)
    assert eng.loudness()[0] is None
    f1 = calls(fresh)
    f2, n2 = calls(fresh), calls(eng)
    assert (n2[1], n2[3]) == (f2[1], f2[3]), (n2[1], n2[3], f2[1], f2[3])
    assert (on[1], on[3]) == (f1[1] + 2, f1[3] + 2), (on[1], on[3], f1[1], f1[3])      # two launches more, one swapped
    for got, want in ((n2[0], f2[0]), (n2[2], f2[2])):
        for x, y in zip(got.audio + got.pcm, want.audio + want.pcm):
            assert x.size and np.array_equal(x, y)
        for a, p in zip(got.audio, got.pcm):
            assert np.array_equal(O.audio_float_to_int16(a), p)
    for e, expect in ((fresh, False), (eng, False), (eng, True)):
        e.set_loudness(-16.0, -2.0) if expect else None
        e.profile_enable(2)
        e.profile_reset()
        e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        names = {r["name"] for r in e.profile() if r["launches"] > 0}
        e.profile_enable(0)
        assert "conv_post_kernel" in names or any("mrf" in n for n in names), names
        assert all((n in names) == expect for n in NAMES), (expect, sorted(names))
        assert ("pcm16_kernel" in names) != expect
    fresh.close()
    eng.close()


def test_off_is_the_parent(emu_lib):
    off_is_parent(lambda: _engine(emu_lib))


# ---- 6. streams untouched
def streams_untouched(eng, cfg, pool_eng=None, pool_cfg=None, multi_speaker=False):
    """The lock-step stream and the pool scenario with the setting off and on, and the one-utterance stream begun with the
    setting on, which then changes and is cleared while the stream is live, against the same stream without it: equal
    chunks, bit for bit."""
    texts = P.emu_texts(cfg, False)[:3]
    ids, nw, nz = K.inputs(cfg)
    sizes_of = lambda k: FIRST if k == 0 else CHUNK      # noqa: E731
    eng.set_loudness(None)
    lock0, _ = K.drain(eng, ids, nw, nz, chunk_frames=sizes_of)
    eng.set_loudness(-16.0, -1.0)
    lock1, _ = K.drain(eng, ids, nw, nz, chunk_frames=sizes_of)
    x = texts[2]
    live = []
    for k, ch in enumerate(eng.stream(x.ids, x.scales, chunk_frames=CHUNK, noise_w=x.nw, noise_z=x.nz)):
        live.append(ch)
        if k == 0:
            eng.set_loudness(-30.0, -6.0)
        if k == 1:
            eng.set_loudness(None)
    base = list(eng.stream(x.ids, x.scales, chunk_frames=CHUNK, noise_w=x.nw, noise_z=x.nz))
    assert len(live) == len(base) > 2

    def same(u, v):
        assert len(u) == len(v) and len(u) > 0
        for (a, p), (b, q) in zip(u, v):
            assert p.size and np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(p, q)

    same(live, base)
    for u, v in zip(lock0, lock1):
        same(u, v)
    pe, pc = pool_eng or eng, pool_cfg or cfg
    pe.set_loudness(None)
    t0 = P.emu_texts(pc, multi_speaker)
    R.play_pool(pe, t0, CHUNK, FIRST)
    pe.set_loudness(-16.0, -1.0)
    t1 = P.emu_texts(pc, multi_speaker)
    R.play_pool(pe, t1, CHUNK, FIRST)
    for u, v in zip(t0, t1):
        assert u.sizes == v.sizes and u.left == v.left
        same(u.chunks, v.chunks)
    pe.set_loudness(None)


def test_streams_untouched(emu_lib, monkeypatch):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, _, eng = _engine(emu_lib)
    streams_untouched(eng, cfg)
    eng.close()


# ---- 8. the command-line tool
def infer_target_lufs(lib, tmp_path):
    """python -m piper_amd.infer --target-lufs on two lines: the WAVs differ from the peak-normalised ones, and the int16
    they hold measures the target (truncation toward zero lowers a level of -20 LUFS by about 0.5 / (0.1 x 32767), 1.3e-3 dB:
    the bound is 0.01 LU) -- unless the ceiling limited the utterance, whose samples then stay under it."""
    import io
    import json
    import wave
    from piper_amd import infer
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    lines = "".join(json.dumps({"phoneme_ids": [int(v) for v in W.synthetic_phoneme_ids(n, s, id_max=39)]}) + "\n"
                    for n, s in ((30, 3), (38, 4)))
    pcm = {}
    for name, extra in (("peak", []), ("lufs", ["--target-lufs", "-20", "--peak-ceiling-db", "-3"])):
        d = tmp_path / name
        args = ["--model", model, "--output-dir", str(d), "--sample-rate", "16000", "--seed", "5", "--noise-scale", "0",
                "--noise-scale-w", "0", "--length-scale", "2.0", "--batch", "2"] + extra
        assert infer.main(args, stdin=io.StringIO(lines), lib=lib) == 0
        pcm[name] = []
        for k in range(2):
            with wave.open(str(d / f"{k}.wav"), "rb") as w:
                assert w.getframerate() == 16000
                pcm[name].append(np.frombuffer(w.readframes(w.getnframes()), np.int16))
    for k in range(2):
        a, b = pcm["peak"][k], pcm["lufs"][k]
        assert a.size == b.size >= 6400 and not np.array_equal(a, b)
        assert int(np.max(np.abs(a.astype(np.int32)))) >= 32766
        t = LC.Truth(b.astype(np.float64) / 32767.0, 16000)
        peak = int(np.max(np.abs(b.astype(np.int32))))
        print(f"line {k}: {t.L:.4f} LUFS, peak {peak}")
        assert not t.flags
        if peak >= int(32767.0 * 10.0 ** (-3.0 / 20.0)) - 1:
            assert peak <= 32767.0 * 10.0 ** (-3.0 / 20.0) and t.L < -20.0
        else:
            assert abs(t.L + 20.0) <= 0.01, t.L


def test_infer_target_lufs(emu_lib, tmp_path):
    infer_target_lufs(emu_lib, tmp_path)


# ---- 9. refusals
def refusals(eng, cfg):
    ids, nw, nz = K.inputs(cfg)
    eng.set_loudness(-19.0, -2.0)
    before = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    x = P.emu_texts(cfg, False)[2]
    base = list(eng.stream(x.ids, x.scales, chunk_frames=CHUNK, noise_w=x.nw, noise_z=x.nz))
    stream = eng.stream(x.ids, x.scales, chunk_frames=CHUNK, noise_w=x.nw, noise_z=x.nz)
    live = [next(stream)]
    bad = [(-40.5, -1.0, "-40.5"), (-4.0, -1.0, "-4.0"), (math.nan, -1.0, "nan"), (math.inf, -1.0, "inf"),
           (-23.0, 0.5, "0.5"), (-23.0, -20.5, "-20.5"), (-23.0, math.nan, "nan"), (-23.0, -math.inf, "inf")]
    for target, ceil, word in bad:
        with pytest.raises(EngineError, match=word.replace(".", r"\.")):
            eng.set_loudness(target, ceil)
        assert eng.loudness() == (-19.0, -2.0)
    live += list(stream)
    assert len(live) == len(base)
    for (a, p), (b, q) in zip(live, base):
        assert np.array_equal(a, b) and np.array_equal(p, q)
    r = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert np.array_equal(r.audio[0], before.audio[0]) and np.array_equal(r.pcm[0], before.pcm[0])
    with pytest.raises(EngineError, match="-50"):
        eng.debug_loudness([np.zeros(8, np.float32)], 16000, -50.0, -1.0)
    with pytest.raises(EngineError, match="3000"):
        eng.debug_loudness([np.zeros(8, np.float32)], 3000)


def test_refusals(emu_lib):
    """Every refused setting names the value and leaves the previous setting, and a live stream, as they were; a voice
    without a header rate has to be told its rate first."""
    cfg, _, eng = _engine(emu_lib)
    refusals(eng, cfg)
    eng.close()
    onnx = Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), lib=emu_lib)
    with pytest.raises(EngineError, match="carries none"):
        onnx.set_loudness(-23.0)
    assert onnx.loudness()[0] is None
    onnx.set_output_rate(None, native=16000)
    onnx.set_loudness(-23.0)
    assert onnx.loudness() == (-23.0, -1.0)
    onnx.close()
