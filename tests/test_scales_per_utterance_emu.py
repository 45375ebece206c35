"""Per-utterance scales (pe_*_scaled, pe_coalescer_create_mixed, the Python and CLI layers above them) on the test-only
emulator build of the engine (tests/emu): every utterance of a batch is computed with its own {noise_scale, length_scale,
noise_w} triple, exactly as a call with that triple alone computes it. The GPU counterpart is
tests/test_gpu_scales_per_utterance.py (-m gpu)."""
import ctypes as C
import io
import json
import os
import subprocess
import threading
import wave

import numpy as np
import pytest

from oracle import vits_oracle as O
from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
GOLD = os.path.join(ROOT, "tests", "golden")

MIXED = np.array([[0.667, 1.0, 0.8], [0.3, 0.7, 0.0], [0.0, 1.5, 1.0], [1.0, 1.2, 0.4]], np.float32)


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _inputs(cfg, lens, seed):
    ids = [W.synthetic_phoneme_ids(T, 40 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate(lens)]
    rng = np.random.default_rng(seed)
    Tm = max(lens)
    return (ids, rng.standard_normal((len(lens), 2, Tm)).astype(np.float32),
            rng.standard_normal((len(lens), cfg.inter, 48 * Tm + 64)).astype(np.float32))


def _lsb(a, b):
    return int(np.max(np.abs(a.astype(np.int32) - b.astype(np.int32)))) if a.size else 0


def test_mixed_scales_match_the_oracle_per_utterance(emu_lib):
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    lens = [9, 5, 12, 7]
    ids, nw, nz = _inputs(cfg, lens, 21)
    r = eng.synthesize_batch(ids, MIXED, noise_w=nw, noise_z=nz)
    durs = eng.durations()
    off = np.concatenate([[0], np.cumsum(lens)])
    wt = O.to_torch(w)
    for i in range(len(ids)):
        sc = tuple(float(v) for v in MIXED[i])
        assert np.array_equal(durs[off[i]:off[i + 1]], O.durations_only(wt, cfg, ids[i], sc, nw[i])), f"utterance {i}"
        o = O.synthesize(w, cfg, ids[i], sc, nw[i], nz[i])
        assert r.audio[i].shape == o["audio"].shape, f"utterance {i}"
        assert np.max(np.abs(r.audio[i] - o["audio"])) < 1e-4, f"utterance {i}"
        assert np.array_equal(O.audio_float_to_int16(r.audio[i]), r.pcm[i])
    # the rates really differ: utterance 2 (length_scale 1.5) has more frames per id than utterance 1 (0.7)
    assert r.frames[2] / lens[2] > r.frames[1] / lens[1]
    eng.close()


def test_repeated_triple_is_bit_identical_to_the_one_triple_entry(emu_lib):
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 77)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    lens = [6, 11, 3]
    ids, nw, nz = _inputs(cfg, lens, 5)
    triple = (0.5, 0.9, 0.6)
    a = eng.synthesize_batch(ids, triple, noise_w=nw, noise_z=nz)
    da = eng.durations()
    b = eng.synthesize_batch(ids, np.tile(np.asarray(triple, np.float32), (3, 1)), noise_w=nw, noise_z=nz)
    assert np.array_equal(da, eng.durations())
    for i in range(3):
        assert np.array_equal(a.audio[i], b.audio[i]) and np.array_equal(a.pcm[i], b.pcm[i])
    # upload + run + fetch with the scaled upload: the same again
    eng.upload(ids, np.tile(np.asarray(triple, np.float32), (3, 1)), noise_w=nw, noise_z=nz)
    eng.run()
    c = eng.fetch()
    for i in range(3):
        assert np.array_equal(a.audio[i], c.audio[i]) and np.array_equal(a.pcm[i], c.pcm[i])
    eng.close()


def test_non_finite_scale_names_the_utterance_and_leaves_the_engine_usable(emu_lib):
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    ids, nw, nz = _inputs(cfg, [7, 4, 9, 5], 3)
    good = MIXED.copy()
    want = eng.synthesize_batch(ids[:2], good[:2], noise_w=nw[:2], noise_z=nz[:2])
    bad = good.copy()
    bad[2, 1] = np.nan
    with pytest.raises(EngineError, match=r"utterance 2: length_scale"):
        eng.synthesize_batch(ids, bad, noise_w=nw, noise_z=nz)
    bad[2, 1] = 1.0
    bad[3, 0] = np.inf
    with pytest.raises(EngineError, match=r"utterance 3: noise_scale"):
        eng.upload(ids, bad)
    # the rejected upload left the previous call's inputs in place: a run on them gives that call's results again
    eng.run()
    again = eng.fetch()
    assert np.array_equal(again.audio[0], want.audio[0]) and np.array_equal(again.audio[1], want.audio[1])
    r = eng.synthesize_batch(ids, good, noise_w=nw, noise_z=nz)
    assert len(r.pcm) == 4 and all(p.size == f * eng.hop for p, f in zip(r.pcm, r.frames))
    # the C entry refuses a NULL scales pointer; a wrong array shape is refused in Python
    i64 = np.ascontiguousarray(np.concatenate(ids), np.int64)
    off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int64)
    res = L.PeResult()
    assert emu_lib.pe_synthesize_batch_scaled(eng._h, i64.ctypes.data_as(C.POINTER(C.c_int64)),
                                              off.ctypes.data_as(C.POINTER(C.c_int64)), 4, None, None, None,
                                              C.byref(res)) != 0
    assert b"null scales" in emu_lib.pe_last_error()
    with pytest.raises(ValueError):
        eng.synthesize_batch(ids, good[:3])
    eng.close()


def test_mixed_coalescer_serves_mixed_rates_in_one_call(emu_lib):
    from piper_amd.group import Coalescer
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    lens = [9, 5, 12, 7, 3, 10]
    ids = [W.synthetic_phoneme_ids(T, 60 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate(lens)]
    rates = [0.7, 1.0, 1.5]
    scales = [(0.0, rates[i % 3], 0.0) for i in range(6)]       # noise scales 0: deterministic
    want = [eng.synthesize(t, s).pcm[0] for t, s in zip(ids, scales)]
    co = Coalescer(eng, max_batch=8, max_wait_us=2000000, mix_scales=True)
    out, errs = [None] * 6, [None] * 6

    def work(i):
        try:
            out[i] = co.synthesize(ids[i], scales[i])
        except EngineError as ex:
            errs[i] = str(ex)

    th = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert errs == [None] * 6
    assert co.stats == (1, 6)
    for i, (pcm, frames, secs, bs) in enumerate(out):
        assert bs == 6
        assert pcm.shape == want[i].shape and _lsb(pcm, want[i]) <= 2, f"request {i}"
    with pytest.raises(EngineError, match="utterance 0: noise_w"):
        co.synthesize(ids[0], (0.0, 1.0, float("nan")))
    co.close()
    eng.close()


def _voice(emu_lib, name="tiny_voice.onnx"):
    from piper_amd.config import PiperConfig
    from piper_amd.voice import PiperVoice
    path = os.path.join(GOLD, name)
    with open(path + ".json", encoding="utf-8") as f:
        cfg = PiperConfig.from_dict(json.load(f))
    return PiperVoice(session=Engine(onnx_path=path, lib=emu_lib), config=cfg)


def test_piper_voice_per_utterance_lists_equal_separate_calls(emu_lib):
    voice = _voice(emu_lib)
    n = voice.session.num_symbols
    ids = [W.synthetic_phoneme_ids(T, 90 + i, id_max=n - 1) for i, T in enumerate((8, 13, 5))]
    ls = [0.8, 1.0, 1.4]
    batch = voice.synthesize_ids_batch_to_raw(ids, length_scale=ls, noise_scale=0.0, noise_w=[0.0, 0.0, 0.0])
    for i in range(3):
        one = voice.synthesize_ids_to_raw(ids[i], length_scale=ls[i], noise_scale=0.0, noise_w=0.0)
        a, b = np.frombuffer(batch[i], np.int16), np.frombuffer(one, np.int16)
        assert a.shape == b.shape and _lsb(a, b) <= 2, f"utterance {i}"
    with pytest.raises(ValueError):
        voice.synthesize_ids_batch_to_raw(ids, length_scale=[1.0, 1.0])
    voice.session.close()


def test_infer_per_line_scale_keys_equal_separate_runs(emu_lib, tmp_path):
    from piper_amd import infer
    model = os.path.join(GOLD, "tiny_voice.onnx")
    n = _voice(emu_lib).session.num_symbols
    ids = [[int(v) for v in W.synthetic_phoneme_ids(T, 70 + i, id_max=n - 1)] for i, T in enumerate((9, 6, 11))]
    own = [{"length_scale": 1.4}, {}, {"length_scale": 0.75, "noise_w": 0.0}]
    base = ["--model", model, "--sample-rate", "16000", "--noise-scale", "0", "--noise-scale-w", "0"]
    lines = [json.dumps(dict(phoneme_ids=p, **o)) for p, o in zip(ids, own)]
    mixed = tmp_path / "mixed"
    assert infer.main(base + ["--output-dir", str(mixed), "--batch", "3"], stdin=io.StringIO("\n".join(lines)),
                      lib=emu_lib) == 0

    def pcm(path):
        with wave.open(str(path), "rb") as f:
            return np.frombuffer(f.readframes(f.getnframes()), np.int16)

    for i, (p, o) in enumerate(zip(ids, own)):
        sep = tmp_path / f"sep{i}"
        args = base + ["--output-dir", str(sep), "--length-scale", str(o.get("length_scale", 1.0))]
        assert infer.main(args, stdin=io.StringIO(json.dumps({"phoneme_ids": p})), lib=emu_lib) == 0
        a, b = pcm(mixed / f"{i}.wav"), pcm(sep / "0.wav")
        assert a.shape == b.shape and _lsb(a, b) <= 2, f"line {i}"
    assert infer.read_scales(lines, (0.1, 0.2, 0.3)) == [(0.1, 1.4, 0.3), None, (0.1, 0.75, 0.0)]
