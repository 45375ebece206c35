"""The true-peak ceiling of the target loudness (pe_set_loudness_ceiling, kernels/true_peak.h) on the test-only emulator
build of the engine: the interpolator's table, the kernel against the f64 restatement of tests/true_peak_case.py, whole
utterances at the native rate and at 8000 / 48000 Hz on poisoned workspaces with both kinds of ceiling, the speculative
one-utterance form, the untouched sample-peak kind, the refusals and the command-line tool. The GPU counterpart is
tests/test_gpu_true_peak.py (-m gpu)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError, Timing, true_peak_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import loudness_case as LC                               # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402
import test_loudness_emu as E                            # noqa: E402
import true_peak_case as TP                              # noqa: E402

TARGET, CEILING = E.TARGET, E.CEILING


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


# ---- 1. the filter
def filter_table(lib):
    """pe_true_peak_filter is the f64 h of tests/resample_case.py for the pair (fs, Q fs) to 1e-14; Q and K as the header
    states them; a rate outside [8000, 48000] is refused by name."""
    for fs, q in ((8000, 24), (16000, 12), (22050, 9), (44100, 5), (48000, 4)):
        Q, Kh, table = true_peak_filter(fs, lib)
        assert (Q, Kh) == (q, TP.K) == (TP.oversample(fs), 18) and table.shape == (q, 36)
        want = TP.filter_f64(fs)
        assert np.max(np.abs(table - want)) <= 1e-14, (fs, np.max(np.abs(table - want)))
        assert abs(table[0, TP.K - 1] - 0.92) <= 1e-12           # phase 0: a lone 1.0 reads 0.92
    for fs in (7999, 48001):
        with pytest.raises(EngineError, match=str(fs)):
            true_peak_filter(fs, lib)


def test_filter(emu_lib):
    filter_table(emu_lib)


# ---- 2. the kernel alone
@pytest.mark.parametrize("fs", TP.RATES)
def test_kernel_against_f64_truth(emu_lib, fs):
    """One ragged batch per rate (true_peak_case.kernel_rows), NaN behind every row's end: every row within the derived
    bound of its f64 true peak, two runs bit-equal, the fs / 4 tone at 0 dB where its samples read -3.01 dB, the impulses
    under their sample peak, silence exactly 0, and a row whose largest excursion straddles two tiles."""
    _, _, eng = E._engine(emu_lib)
    TP.check_kernel(eng, fs)
    eng.close()


# ---- 3. whole utterances
def ceiling_evidence(eng, fs):
    """The fs / 4 tone of the kernel cases converted with the scale of either rule, t measured by the device
    (debug_true_peak): under the sample-peak rule, scale = 32767 C / p, the f64 true peak of the int16 passes C + S / 32767
    (by 3 dB); under the true-peak rule, scale = 32767 C / max(p, t) with the one-ulp lowering, it does not."""
    x = dict(TP.kernel_rows(fs))["quarter"]
    C, S = 10.0 ** (CEILING / 20.0), TP.truncation_slack(fs)
    p, t = float(np.max(np.abs(x))), float(eng.debug_true_peak([x], fs)[0])
    got = {}
    for name, P in (("sample", p), ("true", max(p, t))):
        scale = np.float32(32767.0 * C / P)
        if float(scale) * P > 32767.0 * C:
            scale = np.nextafter(scale, np.float32(0))
        got[name] = TP.true_peak(LC.pcm_of(x, scale).astype(np.float64) / 32767.0, fs)[0]
    print(f"{fs} Hz, fs / 4 tone: p {p:.6f}, device t {t:.6f}; delivered true peak {got['sample']:.5f} under the sample-peak "
          f"rule, {got['true']:.5f} under the true-peak rule (ceiling {C:.5f} + {S / 32767.0:.1e})")
    assert got["true"] <= C + S / 32767.0 < got["sample"], got


def whole_utterances(eng, cfg, rate):
    """The three ragged texts of test_loudness_emu.whole_utterances, with the kind SAMPLE and then TRUE, at T = -23 and
    T = -5: equal floats; in TRUE the reported true peak, scale and flags against the f64 formula with P = max(p, t), the
    int16 the conversion with the reported scale, and the f64 true peak of the delivered int16 under C + S / 32767; at
    T = -5 every measurable utterance is LIMITED.
    The same quantity in SAMPLE does NOT exceed C with these texts: the tiny synthetic voice's waveforms are smooth, so
    their true peak reads below their sample peak (phase 0 of the interpolator has gain 0.92) and P = p. The evidence that
    the sample-peak rule breaks the ceiling and the true-peak rule holds it comes from the fs / 4 row of the kernel cases
    instead (ceiling_evidence): the device's t of that row through both rules."""
    ids, nw, nz = K.inputs(cfg)
    nz = np.ascontiguousarray(np.pad(nz, ((0, 0), (0, 0), (0, max(0, E.STRETCH + 8 - nz.shape[2])))))
    plan = Timing(target_frames=[0, 0, E.STRETCH])
    eng.set_output_rate(rate or 0)
    fs = rate or cfg.sample_rate
    C = 10.0 ** (CEILING / 20.0)
    over_in_sample = 0
    for target in (TARGET, -5.0):
        eng.set_loudness(target, CEILING)
        assert eng.loudness_ceiling()[0] == TP.SAMPLE
        smp = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
        LC.check_delivery(eng, smp, fs, target, CEILING, f"SAMPLE, rate {fs}, T {target}: ")
        assert eng.last_true_peak().size == 0
        for b, pcm in enumerate(smp.pcm):
            d = TP.true_peak(pcm.astype(np.float64) / 32767.0, fs)[0]
            print(f"SAMPLE, rate {fs}, T {target}, utterance {b}: delivered true peak {d:.5f} (ceiling {C:.5f})")
            over_in_sample += d > C
        eng.set_loudness(target, CEILING, true_peak=True)
        assert eng.loudness() == (target, CEILING) and eng.loudness_ceiling() == (TP.TRUE, TP.oversample(fs), TP.K)
        tru = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, timing=plan)
        assert np.array_equal(tru.frames, smp.frames) and int(tru.frames[2]) == E.STRETCH
        for a, b in zip(tru.audio, smp.audio):
            assert a.size and np.array_equal(a.view(np.int32), b.view(np.int32))
        out = TP.check_delivery(eng, tru, fs, target, CEILING, f"TRUE, rate {fs}, T {target}: ")
        if target == -5.0:
            assert all(f & (LC.LIMITED | LC.UNMEASURABLE) for f, _ in out), out
            assert any(f & LC.LIMITED for f, _ in out)
    print(f"rate {fs}: {over_in_sample} deliveries pass the ceiling under the sample-peak rule")
    if not over_in_sample:
        ceiling_evidence(eng, fs)
    eng.set_loudness(None)
    assert eng.loudness_ceiling()[0] == TP.SAMPLE


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


# ---- 4. the speculative one-utterance form
def speculative(make_engine, graphs):
    """test_loudness_emu.speculative with the kind TRUE: after the warm-up every call is the one-graph form with a constant
    launch count, exactly one more than with SAMPLE; both entry points deliver the same bits; switching the kind back and
    forth captures nothing once each has been seen."""
    cfg, _, a = make_engine()
    _, _, b = make_engine()
    one, sc = W.synthetic_phoneme_ids(20, 3, id_max=cfg.n_vocab - 1), (0.667, 1.0, 0.8)
    fs = cfg.sample_rate
    for e in (a, b):
        e.set_loudness(TARGET, CEILING, true_peak=True)
        if graphs:
            e.warmup(1, 32, sample_ids=one)
        else:                                            # (the emulator captures nothing: one call gives the estimate)
            e.synthesize(one, sc)
    runs0 = a.speculation_stats[0]
    launches = []
    for k in range(3):
        r = a.synthesize(one, sc)
        launches.append(a.run_launches)
        TP.check_delivery(a, r, fs, TARGET, CEILING, f"speculative call {k}: ")
        rb = b.synthesize_batch([one], sc)
        assert np.array_equal(r.audio[0], rb.audio[0]) and np.array_equal(r.pcm[0], rb.pcm[0]), k
        assert np.array_equal(a.last_true_peak().view(np.int32), b.last_true_peak().view(np.int32))
    assert a.speculation_stats[0] == runs0 + 3 and len(set(launches)) == 1, (a.speculation_stats, launches)
    # SAMPLE: seen once (its capture), then both kinds alternate on cached graphs
    a.set_loudness(TARGET, CEILING)
    r = a.synthesize(one, sc)
    LC.check_delivery(a, r, fs, TARGET, CEILING, "SAMPLE after TRUE: ")
    c0 = a.graph_stats[1]
    assert not graphs or c0 > 0
    for k in range(2):
        a.set_loudness(TARGET, CEILING, true_peak=True)
        r = a.synthesize(one, sc)
        assert a.run_launches == launches[0], (a.run_launches, launches)
        TP.check_delivery(a, r, fs, TARGET, CEILING, f"TRUE again {k}: ")
        a.set_loudness(TARGET, CEILING)
        r = a.synthesize(one, sc)
        assert a.run_launches == launches[0] - 1, (a.run_launches, launches)
        assert a.last_true_peak().size == 0
        LC.check_delivery(a, r, fs, TARGET, CEILING, f"SAMPLE again {k}: ")
    assert a.graph_stats[1] == c0 and a.speculation_stats[0] == runs0 + 8, (c0, a.graph_stats, a.speculation_stats)
    a.close()
    b.close()


def test_speculative_form(emu_lib):
    speculative(lambda: E._engine(emu_lib), graphs=False)


# ---- 5. SAMPLE is the parent
def sample_is_parent(make_engine):
    """An engine on which the kind was never set and one on which it was set to TRUE and back to SAMPLE make the same
    calls, with the loudness on and with it off: equal bits, equal launch counts, and true_peak_kernel among the launches
    (the profile's per-kernel rows) only while the kind is TRUE and the loudness on."""
    cfg, _, fresh = make_engine()
    _, _, eng = make_engine()
    ids, nw, nz = K.inputs(cfg)
    one, sc = ids[0], (0.667, 0.5, 0.8)

    def calls(e):
        x = e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        lx = e.run_launches
        y = e.synthesize(one, sc)
        return x, lx, y, e.run_launches

    def raw(e, on):                                      # (the parent's call: the kind is never set on `fresh`)
        e._check(e._lib.pe_set_loudness(e._h, int(on), -16.0 if on else 0.0, -2.0 if on else 0.0))

    def same(got, want):
        assert (got[1], got[3]) == (want[1], want[3]), (got[1], got[3], want[1], want[3])
        for g, w in ((got[0], want[0]), (got[2], want[2])):
            for x, y in zip(g.audio + g.pcm, w.audio + w.pcm):
                assert x.size and np.array_equal(x, y)

    # every engine's n-th call is compared with the other's n-th call
    eng.set_loudness(-16.0, -2.0, true_peak=True)
    raw(fresh, True)
    on_true, f1 = calls(eng), calls(fresh)
    assert (on_true[1], on_true[3]) == (f1[1] + 1, f1[3] + 1), (on_true[1], on_true[3], f1[1], f1[3])      # one launch more
    for g, w in ((on_true[0], f1[0]), (on_true[2], f1[2])):
        for x, y in zip(g.audio, w.audio):
            assert x.size and np.array_equal(x, y)
    eng.set_loudness(-16.0, -2.0, true_peak=False)       # SAMPLE, explicitly, with the loudness on
    assert eng.loudness_ceiling()[0] == fresh.loudness_ceiling()[0] == TP.SAMPLE
    same(calls(eng), calls(fresh))
    eng.set_loudness(None, true_peak=True)               # TRUE is remembered while the loudness is off, where it changes nothing
    raw(fresh, False)
    assert eng.loudness_ceiling()[0] == TP.TRUE and eng.loudness()[0] is None
    same(calls(eng), calls(fresh))
    eng.set_loudness(None, true_peak=False)              # SAMPLE, explicitly, with the loudness off
    same(calls(eng), calls(fresh))
    raw(fresh, True)
    for e, kind, expect in ((fresh, False, False), (eng, False, False), (eng, True, True)):
        e.set_loudness(-16.0, -2.0, true_peak=kind) if e is eng else None
        e.profile_enable(2)
        e.profile_reset()
        e.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
        names = {r["name"] for r in e.profile() if r["launches"] > 0}
        e.profile_enable(0)
        assert all(n in names for n in E.NAMES), sorted(names)
        assert ("true_peak_kernel" in names) == expect, (expect, sorted(names))
    fresh.close()
    eng.close()


def test_sample_is_the_parent(emu_lib):
    sample_is_parent(lambda: E._engine(emu_lib))


# ---- 6. refusals and read-back
def refusals(eng, cfg, make_onnx):
    ids, nw, nz = K.inputs(cfg)
    fs = cfg.sample_rate
    assert eng.loudness_ceiling() == (TP.SAMPLE, TP.oversample(fs), TP.K)
    eng.set_loudness(-19.0, -2.0, true_peak=True)
    before = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert eng.last_true_peak().size == 1
    for kind in (2, -1, 7):
        with pytest.raises(EngineError, match=f"kind {kind}"):
            eng._check(eng._lib.pe_set_loudness_ceiling(eng._h, kind))
        assert eng.loudness_ceiling()[0] == TP.TRUE and eng.loudness() == (-19.0, -2.0)
    # the kind may change while a stream is live, and the stream does not see it
    x = P.emu_texts(cfg, False)[2]
    base = list(eng.stream(x.ids, x.scales, chunk_frames=4, noise_w=x.nw, noise_z=x.nz))
    live = []
    for k, ch in enumerate(eng.stream(x.ids, x.scales, chunk_frames=4, noise_w=x.nw, noise_z=x.nz)):
        live.append(ch)
        eng.set_loudness(-19.0, -2.0, true_peak=bool(k & 1))
    assert len(live) == len(base) > 2
    for (a, p), (b, q) in zip(live, base):
        assert np.array_equal(a, b) and np.array_equal(p, q)
    eng.set_loudness(-19.0, -2.0, true_peak=True)
    r = eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert np.array_equal(r.audio[0], before.audio[0]) and np.array_equal(r.pcm[0], before.pcm[0])
    # *n == 0 after a SAMPLE call and after a call with the loudness off
    eng.set_loudness(-19.0, -2.0)
    eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert eng.last_true_peak().size == 0 and eng.last_loudness()[0].size == 1
    eng.set_loudness(None, true_peak=True)
    eng.synthesize(ids[0], (0.667, 0.5, 0.8), noise_w=nw[0], noise_z=nz[0])
    assert eng.last_true_peak().size == 0 and eng.last_loudness()[0].size == 0
    with pytest.raises(EngineError, match="7000"):
        eng.debug_true_peak([np.zeros(8, np.float32)], 7000)
    # a delivered rate outside [8000, 48000] with TRUE and the loudness on is refused wherever it would come about: a voice
    # told a native rate of 7000 Hz (an .onnx carries none)
    onnx = make_onnx()
    onnx.set_output_rate(None, native=7000)
    assert onnx.loudness_ceiling() == (TP.SAMPLE, 0, TP.K)
    onnx.set_loudness(-23.0)                             # the sample-peak kind covers the rate
    with pytest.raises(EngineError, match="7000"):
        onnx._check(onnx._lib.pe_set_loudness_ceiling(onnx._h, TP.TRUE))
    assert onnx.loudness_ceiling()[0] == TP.SAMPLE
    with pytest.raises(EngineError, match="7000"):
        onnx.set_loudness(-23.0, -1.0, true_peak=True)
    assert onnx.loudness_ceiling()[0] == TP.SAMPLE and onnx.loudness() == (-23.0, -1.0)
    onnx.set_loudness(None, true_peak=True)              # off: remembered
    assert onnx.loudness_ceiling()[0] == TP.TRUE
    with pytest.raises(EngineError, match="7000"):
        onnx.set_loudness(-23.0, -1.0, true_peak=True)
    assert onnx.loudness()[0] is None and onnx.loudness_ceiling()[0] == TP.TRUE
    onnx.set_output_rate(None, native=16000)
    onnx.set_loudness(-23.0, -1.0, true_peak=True)
    assert onnx.loudness_ceiling() == (TP.TRUE, 12, TP.K)
    with pytest.raises(EngineError, match="7000"):
        onnx.set_output_rate(None, native=7000)
    assert onnx.output_rate == 16000 and onnx.loudness_ceiling() == (TP.TRUE, 12, TP.K)
    onnx.close()


def test_refusals(emu_lib):
    """An unknown kind names the value and changes nothing; the kind may change under a live stream; the report is empty
    after a SAMPLE call; a rate the measure does not cover is refused by set_loudness, set_loudness_ceiling and
    set_output_rate alike."""
    cfg, _, eng = E._engine(emu_lib)
    refusals(eng, cfg, lambda: Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), lib=emu_lib))
    eng.close()


# ---- 7. the command-line tool
def infer_true_peak(lib, tmp_path):
    """python -m piper_amd.infer --target-lufs -5 --peak-ceiling-db -3 --true-peak on two lines: the f64 true peak of the
    WAVs' int16 lies under C + S / 32767, which at least one of the WAVs written without --true-peak passes."""
    import io
    import json
    import wave
    from piper_amd import infer
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    lines = "".join(json.dumps({"phoneme_ids": [int(v) for v in W.synthetic_phoneme_ids(n, s, id_max=39)]}) + "\n"
                    for n, s in ((30, 3), (38, 4)))
    C, S = 10.0 ** (-3.0 / 20.0), TP.truncation_slack(16000)
    pcm = {}
    for name, extra in (("sample", []), ("true", ["--true-peak"])):
        d = tmp_path / name
        args = ["--model", model, "--output-dir", str(d), "--sample-rate", "16000", "--seed", "5", "--noise-scale", "0",
                "--noise-scale-w", "0", "--length-scale", "2.0", "--batch", "2", "--target-lufs", "-5",
                "--peak-ceiling-db", "-3"] + extra
        assert infer.main(args, stdin=io.StringIO(lines), lib=lib) == 0
        pcm[name] = []
        for k in range(2):
            with wave.open(str(d / f"{k}.wav"), "rb") as w:
                assert w.getframerate() == 16000
                pcm[name].append(np.frombuffer(w.readframes(w.getnframes()), np.int16))
    broke = 0
    for k in range(2):
        a, b = pcm["sample"][k], pcm["true"][k]
        ta, tb = (TP.true_peak(v.astype(np.float64) / 32767.0, 16000)[0] for v in (a, b))
        print(f"line {k}: delivered true peak {ta:.5f} with the sample-peak ceiling, {tb:.5f} with --true-peak (ceiling {C:.5f})")
        assert a.size == b.size >= 6400
        assert tb <= C + S / 32767.0
        broke += ta > C + S / 32767.0 and not np.array_equal(a, b)
    assert broke >= 1, "no line passes the ceiling under the sample-peak rule: these lines show nothing"


def test_infer_true_peak(emu_lib, tmp_path):
    infer_true_peak(emu_lib, tmp_path)
