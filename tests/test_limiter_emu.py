"""The look-ahead limiter of the target loudness (pe_set_loudness_limiter, kernels/limiter.h) on the test-only emulator build
of the engine: the window, the kernel against the f64 restatement of tests/limiter_case.py, whole utterances at the native
rate and at 8000 / 48000 Hz on poisoned workspaces, the clicks row, the speculative one-utterance form, the untouched
limiter-off path, the refusals and the command-line tool. The GPU counterpart is tests/test_gpu_limiter.py (-m gpu)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError, Timing, limiter_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import limiter_case as LM                                # noqa: E402
import loudness_case as LC                               # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402
import test_loudness_emu as E                            # noqa: E402

TARGET, CEILING, MS = -8.0, LM.CEILING, 5.0
NAMES_ON = ("loudness_seg_kernel", "loudness_gain_kernel", "limiter_kernel")


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


# ---- 1. the window
def window_table(lib):
    """pe_limiter_window is the f64 window of tests/limiter_case.py to 1e-15, W as the header states it; a window or a rate
    outside the range is refused by name."""
    for fs, ms, w in ((8000, 1.0, 8), (48000, 10.0, 480), (22050, 5.0, 110), (16000, 2.5, 40)):
        Wd, h = limiter_window(fs, ms, lib)
        Wt, ht = LM.window(fs, ms)
        assert Wd == Wt == w and h.shape == (2 * w + 1,)
        assert np.max(np.abs(h - ht)) <= 1e-15 and abs(h.sum() - 1.0) <= 1e-14 and h.min() > 0.0
    for ms in (0.5, 10.5, float("nan"), float("inf")):
        with pytest.raises(EngineError, match="nan|inf|0.5|10.5"):
            limiter_window(16000, ms, lib)
    with pytest.raises(EngineError, match="3000"):
        limiter_window(3000, 5.0, lib)


def test_window(emu_lib):
    window_table(emu_lib)


# ---- 2. the kernel alone
@pytest.mark.parametrize("ms", LM.WINDOWS)
@pytest.mark.parametrize("fs", LM.RATES)
def test_kernel_against_f64_truth(emu_lib, fs, ms):
    """One ragged batch per rate and window (limiter_case.kernel_rows), NaN behind every row's end: the envelope within the
    derived bound of the f64 one, two runs bit-equal, e <= r, e == 1 away from every peak, the int16 the f32 restatement and
    under the ceiling, the envelope continuous across the tile seam."""
    _, _, eng = E._engine(emu_lib)
    LM.check_kernel(eng, fs, ms)
    eng.close()


@pytest.mark.parametrize("ms", LM.WINDOWS)
@pytest.mark.parametrize("fs", LM.RATES)
def test_kernel_true_peak_against_f64_truth(emu_lib, fs, ms):
    """The same batches under the true-peak ceiling (true_peak_v_kernel, limiter_true_kernel, true_peak_kernel on z,
    pcm16_trim_kernel): the envelope from max(|x|, v[i - 1], v[i]) within its bound, the int16 against the conversion of
    z with the trimmed f64 scale, its f64 true peak under C + S / 32767."""
    _, _, eng = E._engine(emu_lib)
    LM.check_kernel_true(eng, fs, ms)
    eng.close()


# ---- 3. whole utterances
def whole_utterances(eng, cfg, rate):
    for kind in (False, True):
        whole_utterances_kind(eng, cfg, rate, kind)


def whole_utterances_kind(eng, cfg, rate, kind):
    """The three ragged texts of test_loudness_emu.whole_utterances at T = -8 under -1 dB, limiter off and then on: equal
    floats, the report and the int16 against the f64 envelope, every shaped row under the ceiling and strictly nearer the
    target than without the limiter; at T = -40, where nothing conflicts, the limiter changes no bit."""
    ids, nw, nz = K.inputs(cfg)
    nz = np.ascontiguousarray(np.pad(nz, ((0, 0), (0, 0), (0, max(0, E.STRETCH + 8 - nz.shape[2])))))
    plan = Timing(target_frames=[0, 0, E.STRETCH])
    eng.set_output_rate(rate or 0)
    fs = rate or cfg.sample_rate
    eng.set_loudness(TARGET, CEILING, true_peak=kind)
    assert eng.loudness_limiter()[0] is False
    off = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
    off_flags = eng.last_loudness()[3].copy()
    assert eng.last_limiter()[0].size == 0
    eng.set_loudness(TARGET, CEILING, true_peak=kind, limiter=True, limiter_ms=MS)
    assert eng.loudness() == (TARGET, CEILING) and eng.loudness_limiter() == (True, MS, LM.window(fs, MS)[0])
    assert eng.loudness_ceiling()[0] == int(kind)
    on = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
    assert np.array_equal(on.frames, off.frames) and int(on.frames[2]) == E.STRETCH
    flags = LM.check_delivery(eng, on, off, fs, TARGET, CEILING, MS, f"rate {fs}, kind {int(kind)}: ", kind=int(kind))
    assert any(f & LM.SHAPED for f in flags), flags
    assert all((f & ~LM.SHAPED) == g for f, g in zip(flags, off_flags)), (flags, off_flags)
    for target in (-40.0,):
        eng.set_loudness(target, CEILING, true_peak=kind)
        a = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
        eng.set_loudness(target, CEILING, true_peak=kind, limiter=True, limiter_ms=MS)
        b = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
        f = LM.check_delivery(eng, b, a, fs, target, CEILING, MS, f"rate {fs}, kind {int(kind)}, T {target}: ", kind=int(kind))
        assert not any(v & (LM.SHAPED | LC.LIMITED) for v in f), f
        for x, y in zip(a.pcm, b.pcm):
            assert x.size and np.array_equal(x, y)
    eng.set_loudness(None)
    assert eng.loudness_limiter()[0] is False


@pytest.mark.parametrize("rate", [0, 8000, 48000])
def test_whole_utterances(emu_lib, monkeypatch, rate):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, _, eng = E._engine(emu_lib)
    whole_utterances(eng, cfg, rate)
    eng.close()


def test_whole_utterances_f16x3(emu_lib, monkeypatch):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    monkeypatch.setenv("PIPER_HIP_MATRIX", "f16x3")
    cfg, _, eng = E._engine(emu_lib)
    whole_utterances(eng, cfg, 0)
    eng.close()


# ---- 4. the clicks row
def clicks(eng):
    """Noise at 0.1 with four clicks of 0.9: at -16 and -12 LUFS under -1 dB the limiter-off rule falls at least 2 dB short of
    the target, the limiter at most 0.5 dB."""
    for fs in LM.RATES:
        for target in (-16.0, -12.0):
            on, off = LM.check_clicks(eng, fs, target)
            assert off >= 2.0, (fs, target, off)
            assert -0.01 <= on <= 0.5, (fs, target, on)


def test_clicks(emu_lib):
    _, _, eng = E._engine(emu_lib)
    clicks(eng)
    eng.close()


# ---- 5. the speculative one-utterance form
def speculative(make_engine, graphs):
    """Two engines with equal seeds make the same calls, one with the limiter and one without: after the warm-up every call
    is the one-graph form with a constant launch count, the same on both (limiter_kernel stands in pcm16_gain_kernel's
    place); the floats are equal and the limiter's delivery holds against the truth; switching the limiter on and off
    captures nothing once each has been seen; a new window captures once."""
    cfg, _, a = make_engine()
    _, _, b = make_engine()
    one, sc = W.synthetic_phoneme_ids(20, 3, id_max=cfg.n_vocab - 1), (0.667, 1.0, 0.8)
    fs = cfg.sample_rate
    for e in (a, b):
        e.set_loudness(TARGET, CEILING, limiter=e is a, limiter_ms=MS)
        if graphs:
            e.warmup(1, 32, sample_ids=one)
        else:                                            # (the emulator captures nothing: one call gives the estimate)
            e.synthesize(one, sc)
    runs0 = a.speculation_stats[0]
    launches = []
    for k in range(3):
        r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
        launches.append(a.run_launches)
        assert b.run_launches == a.run_launches, (k, a.run_launches, b.run_launches)
        assert a.last_limiter()[0].size == 1 and b.last_limiter()[0].size == 0
        LM.check_delivery(a, r, rb, fs, TARGET, CEILING, MS, f"speculative call {k}: ")
    assert a.speculation_stats[0] == runs0 + 3 and len(set(launches)) == 1, (a.speculation_stats, launches)
    # off: seen once (its capture), then both settings alternate on cached graphs
    a.set_loudness(TARGET, CEILING)
    r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
    assert np.array_equal(r.pcm[0], rb.pcm[0]) and a.run_launches == launches[0]
    c0 = a.graph_stats[1]
    assert not graphs or c0 > 0
    for k in range(2):
        a.set_loudness(TARGET, CEILING, limiter=True, limiter_ms=MS)
        r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
        assert a.run_launches == launches[0]
        LM.check_delivery(a, r, rb, fs, TARGET, CEILING, MS, f"on again {k}: ")
        a.set_loudness(TARGET, CEILING)
        r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
        assert a.run_launches == launches[0] and a.last_limiter()[0].size == 0
        assert np.array_equal(r.audio[0], rb.audio[0]) and np.array_equal(r.pcm[0], rb.pcm[0])
    assert a.graph_stats[1] == c0 and a.speculation_stats[0] == runs0 + 8, (c0, a.graph_stats, a.speculation_stats)
    c0 = None
    # the four settings -- either kind of ceiling, the limiter off and on -- alternate on cached graphs once each has been
    # seen; the true-peak ceiling costs one launch without the limiter and three more with it
    four = ((False, False, 0), (False, True, 0), (True, False, 1), (True, True, 3))
    for tp, lim, _ in four:
        for e in (a, b):
            e.set_loudness(TARGET, CEILING, true_peak=tp, limiter=lim and e is a, limiter_ms=MS)
        a.synthesize(one, sc), b.synthesize(one, sc)
    c0 = a.graph_stats[1]
    for k in range(2):
        for tp, lim, extra in four:
            for e in (a, b):
                e.set_loudness(TARGET, CEILING, true_peak=tp, limiter=lim and e is a, limiter_ms=MS)
            r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
            assert a.run_launches == launches[0] + extra, (tp, lim, a.run_launches, launches)
            if lim:
                LM.check_delivery(a, r, rb, fs, TARGET, CEILING, MS, f"four settings {k}, kind {int(tp)}: ", kind=int(tp))
            else:
                assert np.array_equal(r.pcm[0], rb.pcm[0]) and a.last_limiter()[0].size == 0
    assert a.graph_stats[1] == c0, (c0, a.graph_stats)
    for e in (a, b):
        e.set_loudness(TARGET, CEILING)
    cw = a.graph_stats[1]
    # a new window: the graphs go, the next call captures, the one after it does not
    a.set_loudness(TARGET, CEILING, limiter=True, limiter_ms=2.0)
    r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
    c1 = a.graph_stats[1]
    assert (c1 > cw) == bool(graphs), (cw, c1)
    LM.check_delivery(a, r, rb, fs, TARGET, CEILING, 2.0, "2 ms: ")
    r, rb = a.synthesize(one, sc), b.synthesize(one, sc)
    assert a.graph_stats[1] == c1 and a.run_launches == launches[0]
    LM.check_delivery(a, r, rb, fs, TARGET, CEILING, 2.0, "2 ms again: ")
    a.close()
    b.close()


def test_speculative_form(emu_lib):
    speculative(lambda: E._engine(emu_lib), graphs=False)


# ---- 6. off is the parent
def off_is_parent(make_engine):
    """An engine on which the limiter was never set and one on which it was set and cleared make the same calls, with the
    loudness on (both kinds of ceiling) and off: equal bits, equal reported scales, equal launch counts, and limiter_kernel
    among the launches (the profile's per-kernel rows) only while the limiter and the loudness are on -- in
    pcm16_gain_kernel's place, with the same count."""
    cfg, _, fresh = make_engine()
    _, _, eng = make_engine()
    ids, nw, nz = K.inputs(cfg)
    one, sc = ids[0], (0.667, 0.5, 0.8)

    def calls(e):
        x = e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        lx, sx = e.run_launches, [v.copy() for v in e.last_loudness()]
        y = e.synthesize(one, sc)
        return x, lx, y, e.run_launches, sx

    def raw(e, on, kind=0):                              # (the parent's calls: the limiter is never set on `fresh`)
        e._check(e._lib.pe_set_loudness(e._h, 0, 0.0, 0.0))
        e._check(e._lib.pe_set_loudness_ceiling(e._h, kind))
        e._check(e._lib.pe_set_loudness(e._h, int(on), -8.0 if on else 0.0, -2.0 if on else 0.0))

    def same(got, want):
        assert (got[1], got[3]) == (want[1], want[3]), (got[1], got[3], want[1], want[3])
        for g, w in ((got[0], want[0]), (got[2], want[2])):
            for x, y in zip(g.audio + g.pcm, w.audio + w.pcm):
                assert x.size and np.array_equal(x, y)
        for x, y in zip(got[4], want[4]):
            assert np.array_equal(x, y)

    eng.set_loudness(-8.0, -2.0, limiter=True, limiter_ms=MS)
    raw(fresh, True)
    on, f1 = calls(eng), calls(fresh)
    assert (on[1], on[3]) == (f1[1], f1[3]), (on[1], on[3], f1[1], f1[3])      # three launches, as without it
    assert any(f & LM.SHAPED for f in on[4][3]) and not any(f & LM.SHAPED for f in f1[4][3])
    eng.set_loudness(-8.0, -2.0, true_peak=True, limiter=True, limiter_ms=MS)
    raw(fresh, True)
    on4, f4 = calls(eng), calls(fresh)
    assert (on4[1], on4[3]) == (f4[1] + 3, f4[3] + 3), (on4[1], on4[3], f4[1], f4[3])      # six launches against three
    for kind in (False, True):
        eng.set_loudness(-8.0, -2.0, true_peak=kind)     # limiter off, loudness on
        raw(fresh, True, int(kind))
        assert eng.loudness_limiter()[0] is False
        same(calls(eng), calls(fresh))
    eng.set_loudness(None, limiter=True, limiter_ms=MS)  # remembered while the loudness is off, where it changes nothing
    raw(fresh, False)
    assert eng.loudness_limiter()[:2] == (True, MS) and eng.loudness()[0] is None
    same(calls(eng), calls(fresh))
    eng.set_loudness(None)
    same(calls(eng), calls(fresh))
    raw(fresh, True)
    for e, lim, expect in ((fresh, False, False), (eng, False, False), (eng, True, True)):
        e.set_loudness(-8.0, -2.0, limiter=lim, limiter_ms=MS) if e is eng else None
        e.profile_enable(2)
        e.profile_reset()
        e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        names = {r["name"] for r in e.profile() if r["launches"] > 0}
        e.profile_enable(0)
        assert all(n in names for n in (NAMES_ON if expect else E.NAMES)), sorted(names)
        assert ("limiter_kernel" in names) == expect and ("pcm16_gain_kernel" in names) != expect, (expect, sorted(names))
        assert not names & {"limiter_true_kernel", "true_peak_v_kernel", "pcm16_trim_kernel"}, sorted(names)
    eng.set_loudness(-8.0, -2.0, true_peak=True, limiter=True, limiter_ms=MS)
    eng.profile_enable(2)
    eng.profile_reset()
    eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    names = {r["name"] for r in eng.profile() if r["launches"] > 0}
    eng.profile_enable(0)
    assert {"true_peak_v_kernel", "limiter_true_kernel", "true_peak_kernel", "pcm16_trim_kernel"} <= names, sorted(names)
    assert not names & {"limiter_kernel", "pcm16_gain_kernel"}, sorted(names)
    fresh.close()
    eng.close()


def test_off_is_the_parent(emu_lib):
    off_is_parent(lambda: E._engine(emu_lib))


# ---- 7. refusals and read-back
def refusals(eng, cfg, make_onnx):
    ids, nw, nz = K.inputs(cfg)
    fs = cfg.sample_rate
    assert eng.loudness_limiter() == (False, 5.0, LM.window(fs, 5.0)[0])
    eng.set_loudness(-8.0, -2.0, limiter=True, limiter_ms=3.0)
    before = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert eng.last_limiter()[0].size == 1
    state = (True, 3.0, LM.window(fs, 3.0)[0])
    for ms, name in ((0.99, "0.99"), (10.01, "10.01"), (float("nan"), "nan"), (float("inf"), "inf"), (-5.0, "-5")):
        with pytest.raises(EngineError, match=name):
            eng._check(eng._lib.pe_set_loudness_limiter(eng._h, 1, ms))
        with pytest.raises(EngineError, match=name):
            eng.set_loudness(-19.0, -3.0, limiter=True, limiter_ms=ms)
        assert eng.loudness_limiter() == state and eng.loudness() == (-8.0, -2.0)
    # a refused call with the loudness to be switched off leaves the loudness on as well
    with pytest.raises(EngineError, match="12"):
        eng.set_loudness(None, limiter=True, limiter_ms=12.0)
    assert eng.loudness_limiter() == state and eng.loudness() == (-8.0, -2.0)
    # either kind of ceiling goes with the limiter, in either order
    eng._check(eng._lib.pe_set_loudness_ceiling(eng._h, 1))
    assert eng.loudness_limiter() == state and eng.loudness_ceiling()[0] == 1
    eng.set_loudness(-8.0, -2.0, true_peak=True)
    eng._check(eng._lib.pe_set_loudness_limiter(eng._h, 1, 3.0))
    assert eng.loudness_limiter() == state and eng.loudness_ceiling()[0] == 1
    eng.set_loudness(-8.0, -2.0, limiter=True, limiter_ms=3.0)
    assert eng.loudness_ceiling()[0] == 0
    # the setting may change while a stream is live, and the stream does not see it
    x = P.emu_texts(cfg, False)[2]
    base = list(eng.stream(x.ids, x.scales, chunk_frames=4, noise_w=x.nw, noise_z=x.nz))
    live = []
    for k, ch in enumerate(eng.stream(x.ids, x.scales, chunk_frames=4, noise_w=x.nw, noise_z=x.nz)):
        live.append(ch)
        eng.set_loudness(-8.0, -2.0, limiter=bool(k & 1), limiter_ms=3.0)
    assert len(live) == len(base) > 2
    for (a, p), (b, q) in zip(live, base):
        assert np.array_equal(a, b) and np.array_equal(p, q)
    eng.set_loudness(-8.0, -2.0, limiter=True, limiter_ms=3.0)
    r = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert np.array_equal(r.audio[0], before.audio[0]) and np.array_equal(r.pcm[0], before.pcm[0])
    # *n == 0 after a call without the limiter and after a call with the loudness off
    eng.set_loudness(-8.0, -2.0)
    eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert eng.last_limiter()[0].size == 0 and eng.last_loudness()[0].size == 1
    eng.set_loudness(None, limiter=True)
    eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert eng.last_limiter()[0].size == 0 and eng.last_loudness()[0].size == 0
    with pytest.raises(EngineError, match="12.0"):
        eng.debug_limiter([np.ones(8, np.float32)], fs, [1.0], -1.0, 0, 12.0)
    with pytest.raises(EngineError, match="kind 2"):
        eng.debug_limiter([np.ones(8, np.float32)], fs, [1.0], -1.0, 2, 5.0)
    with pytest.raises(EngineError, match="7000"):
        eng.debug_limiter([np.ones(8, np.float32)], 7000, [1.0], -1.0, 1, 5.0)
    # a delivered rate at which the window passes 480 samples is refused wherever it would come about: a voice told a native
    # rate of 96000 Hz (an .onnx carries none)
    onnx = make_onnx()
    onnx.set_output_rate(None, native=96000)
    onnx.set_loudness(-23.0, -1.0, limiter=True, limiter_ms=5.0)       # 480 samples
    with pytest.raises(EngineError, match="96000"):
        onnx.set_loudness(-23.0, -1.0, limiter=True, limiter_ms=6.0)
    assert onnx.loudness_limiter() == (True, 5.0, 480)
    onnx.set_output_rate(None, native=16000)
    onnx.set_loudness(-23.0, -1.0, limiter=True, limiter_ms=10.0)
    with pytest.raises(EngineError, match="96000"):
        onnx.set_output_rate(None, native=96000)
    assert onnx.output_rate == 16000 and onnx.loudness_limiter() == (True, 10.0, 160)
    # the true-peak ceiling with the limiter follows the true-peak ceiling's rate refusals
    onnx.set_loudness(None)
    onnx.set_output_rate(None, native=7000)
    onnx.set_loudness(-23.0, -1.0, limiter=True, limiter_ms=5.0)       # the sample-peak kind covers the rate
    with pytest.raises(EngineError, match="7000"):
        onnx.set_loudness(-23.0, -1.0, true_peak=True, limiter=True, limiter_ms=5.0)
    assert onnx.loudness_ceiling()[0] == 0 and onnx.loudness() == (-23.0, -1.0) and onnx.loudness_limiter()[:2] == (True, 5.0)
    with pytest.raises(EngineError, match="7000"):
        onnx._check(onnx._lib.pe_set_loudness_ceiling(onnx._h, 1))
    onnx.set_output_rate(None, native=16000)
    onnx.set_loudness(-23.0, -1.0, true_peak=True, limiter=True, limiter_ms=5.0)
    with pytest.raises(EngineError, match="7000"):
        onnx.set_output_rate(None, native=7000)
    assert onnx.output_rate == 16000 and onnx.loudness_ceiling()[0] == 1 and onnx.loudness_limiter() == (True, 5.0, 80)
    onnx.close()


def test_refusals(emu_lib):
    """A window outside [1, 10] ms or not finite names the value and changes nothing (the loudness that was to be switched off
    included); the limiter goes with either kind of ceiling and follows the true-peak ceiling's rate refusals; the setting may change under a live stream; the report is empty after a call without the limiter; a
    rate at which the window is too long is refused by set_loudness, set_loudness_limiter and set_output_rate alike."""
    cfg, _, eng = E._engine(emu_lib)
    refusals(eng, cfg, lambda: Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), lib=emu_lib))
    eng.close()


# ---- 8. the command-line tool
def infer_limiter(lib, tmp_path):
    """python -m piper_amd.infer --target-lufs -8 --peak-ceiling-db -3 --limiter on two lines: the WAVs stay under the ceiling
    and, where the two differ, the limiter's lies nearer the target."""
    import io
    import json
    import wave
    from piper_amd import infer
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    lines = "".join(json.dumps({"phoneme_ids": [int(v) for v in W.synthetic_phoneme_ids(n, s, id_max=39)]}) + "\n"
                    for n, s in ((30, 3), (38, 4)))
    C = float(LM.ceiling_f32(-3.0))
    pcm = {}
    for name, extra in (("off", []), ("on", ["--limiter", "--limiter-ms", "4"])):
        d = tmp_path / name
        args = ["--model", model, "--output-dir", str(d), "--sample-rate", "16000", "--seed", "5", "--noise-scale", "0",
                "--noise-scale-w", "0", "--length-scale", "2.0", "--batch", "2", "--target-lufs", "-8",
                "--peak-ceiling-db", "-3"] + extra
        assert infer.main(args, stdin=io.StringIO(lines), lib=lib) == 0
        pcm[name] = []
        for k in range(2):
            with wave.open(str(d / f"{k}.wav"), "rb") as w:
                assert w.getframerate() == 16000
                pcm[name].append(np.frombuffer(w.readframes(w.getnframes()), np.int16))
    shaped = 0
    for k in range(2):
        a, b = pcm["off"][k], pcm["on"][k]
        assert a.size == b.size >= 6400
        assert int(np.max(np.abs(b.astype(np.int32)))) <= 32767.0 * C
        if not np.array_equal(a, b):
            la, lb = LM.delivered_loudness(a, 16000), LM.delivered_loudness(b, 16000)
            print(f"line {k}: {la.L:.3f} LUFS without the limiter, {lb.L:.3f} with it (target -8)")
            assert la.L < lb.L <= -8.0 + 0.01
            shaped += 1
    assert shaped >= 1, "no line is shaped: these lines show nothing"


def test_infer_limiter(emu_lib, tmp_path):
    infer_limiter(emu_lib, tmp_path)
