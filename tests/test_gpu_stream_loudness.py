"""Streams at a target loudness on the MI355X (run with -m gpu): pe_set_stream_loudness through
piper_amd.engine.Engine.set_stream_loudness -- the kernel rows and the rule through the debug entry at four rates, and batch
streams, the one-utterance stream and the pool on the tiny voice with the inputs of tests/emu/stream_batch_case.py (6, 14 and
23 ids, chunks of 4 frames and of 1). The contract is restated in f64 in tests/stream_loudness_case.py. The twin of
tests/test_stream_loudness_emu.py, which runs the same cases on the emulator with poisoned state."""
import os
import sys

import numpy as np
import pytest

from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import loudness_case as LC                               # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_gain_case as G                             # noqa: E402
import stream_loudness_case as S                         # noqa: E402
import stream_pool_case as P                             # noqa: E402

pytestmark = pytest.mark.gpu

T, CEIL, RAMP = -20.0, -1.0, 64
CHUNKS = (4, 1)


_engines = {}


def _engine(preset="tiny", own=False):
    """(cfg, engine) on device 0. The shared one per voice serves the tests that leave the handle as they found it."""
    from piper_amd.engine import Engine
    cfg = W.preset(preset)
    if own:
        return cfg, Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    if preset not in _engines:
        _engines[preset] = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    return cfg, _engines[preset]


@pytest.fixture(scope="module")
def tiny():
    cfg, eng = _engine()
    return cfg, eng, K.inputs(cfg)


# ---- 1. kernel rows through the debug entry
@pytest.mark.parametrize("fs", LC.RATES)
def test_kernel_rows(tiny, fs):
    S.check_kernel(tiny[1], fs)


# ---- 2. the rule
@pytest.mark.parametrize("fs", (8000, 22050))
def test_rule(tiny, fs):
    S.check_rule(tiny[1], fs)


# ---- 4. the feature does what it is for
@pytest.mark.parametrize("fs", (16000, 48000))
def test_levels_meet_the_target_where_the_running_peak_cannot(tiny, fs):
    S.check_feature(tiny[1], fs)


# ---- 3. engine streams
_base = {}


def _batch(eng, inputs, chunk, rate, prior):
    """The ragged batch stream in the default mode (once per rate and chunk size), then in the loudness mode."""
    ids, nw, nz = inputs
    if (rate, chunk) not in _base:
        eng.set_stream_gain("chunk")
        _base[(rate, chunk)] = G.drain(eng, ids, nw, nz, chunk, K.SCALES)[0]
    base = _base[(rate, chunk)]
    fs = eng.output_rate
    eng.set_stream_loudness(T, CEIL, prior, RAMP * 1000.0 / fs)
    assert eng.stream_gain == ("loudness", 0.0, RAMP) and eng.stream_loudness == (True, T, CEIL, prior, RAMP)
    per = S.drain_batch(eng, ids, nw, nz, chunk, K.SCALES)
    streams = S.check_streams(per, fs, T, CEIL, prior, RAMP, ("batch", rate, chunk))
    for b in range(len(ids)):                              # the floats do not depend on the mode
        mine = [a for a, _, _ in per[b] if a.size]
        assert len(mine) == len(base[b]) and all(np.array_equal(a, a0) for a, (a0, _) in zip(mine, base[b])), b
    eng.set_stream_gain("chunk")
    return per, streams


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("rate", (None, 8000))
def test_batch_stream(chunk, rate):
    cfg, eng = _engine(own=True)
    inputs = K.inputs(cfg)
    ids, nw, nz = inputs
    if rate:
        eng.set_output_rate(rate)
    fs = eng.output_rate
    per, streams = _batch(eng, inputs, chunk, rate, None)
    h = (fs + 5) // 10
    n = [s.X.size for s in streams]
    print(f"\nsamples per stream at {fs} Hz: {n} (h = {h})")
    assert n[0] < n[1] < 4 * h and n[2] >= 6 * h, n       # streams that stay SHORT, and one that goes on to three blocks
    assert streams[0].last[3] & S.SHORT and not streams[2].last[3] & S.SHORT
    # finished rows kept reporting their end state (Stream.chunk on every empty chunk); there were such calls
    assert sum(1 for a, _, _ in per[0] if a.size == 0) >= 3
    # the whole-utterance call on the same inputs: not gated, the floats of the two paths differ by the stream's tolerance
    eng.set_loudness(T, CEIL)
    eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    Lw = eng.last_loudness()[0]
    eng.set_loudness(None)
    for b, s in enumerate(streams):
        print(f"rate {fs}, chunks of {chunk}, utterance {b}: L_last {s.last[0]:.5f}, pe_last_loudness {float(Lw[b]):.5f}, "
              f"difference {s.last[0] - float(Lw[b]):+.6f} LU")
    # with a prior: the SHORT stream follows it to its end
    if chunk == K.CHUNK:
        per, streams = _batch(eng, inputs, chunk, rate, -30.0)
        assert all(rep[3] & S.PRIOR for a, _, rep in per[0] if a.size) and not streams[2].last[3] & S.PRIOR
    eng.close()


@pytest.mark.parametrize("chunk", CHUNKS)
def test_one_utterance_stream(tiny, chunk):
    """pe_stream_next converts on the host, with an f64 serial filter: the same rule, the same reports; and chunk k of
    utterance b of the batch stream reports what the one-utterance stream does."""
    cfg, eng, (ids, nw, nz) = tiny
    fs = eng.output_rate
    eng.set_stream_loudness(T, CEIL, None, RAMP * 1000.0 / fs)
    per = S.drain_batch(eng, ids, nw, nz, chunk, K.SCALES)
    streams = []
    for b in range(len(ids)):
        calls, end = S.drain_one(eng, ids[b], K.SCALES[b], nw[b], nz[b], chunk)
        s = S.Stream(fs, T, CEIL, None, RAMP)
        for k, (a, pc, rep) in enumerate(calls):
            s.chunk(a, pc, rep, ("one", b, k), last=k == len(calls) - 1)
        assert S.tuple_eq(end, s.last), (b, end, s.last)          # the call that ended it delivered nothing: the end state
        streams.append(s)
        mine = [c for c in per[b] if c[0].size]
        assert len(mine) == len(calls), b
        for k, ((a, pc, rep), (a1, pc1, rep1)) in enumerate(zip(mine, calls)):
            assert a.shape == a1.shape and np.max(np.abs(a - a1)) < 1e-5, (b, k)
            assert rep[3] == rep1[3] and rep[2] == pytest.approx(rep1[2], abs=1e-5), (b, k, rep, rep1)
            if np.isfinite(rep[0]):
                assert abs(rep[0] - rep1[0]) <= 2 * S.L_TOL and abs(rep[1] - rep1[1]) <= 2 * S.SCALE_TOL * rep[1], (b, k, rep, rep1)
    S.assert_exclusions(streams, f"one utterance, chunks of {chunk}")
    eng.set_stream_gain("chunk")


def test_pool_state_is_per_slot_and_resident():
    """Three slots: a newcomer joins two residents in mid-stream; a whole-utterance call, a batch that grows both
    workspaces and a join without room happen between two chunks; a finished tenant's slot and
    a departed listener's slot are reused, and the new tenants start from nothing."""
    cfg, eng = _engine("tiny-ms", own=True)
    big = [W.synthetic_phoneme_ids(n, 90 + i, id_max=cfg.n_vocab - 1) for i, n in enumerate((136, 3, 4, 5))]
    t3 = P.emu_texts(cfg, True)[3]

    def between(k):
        if k == 0:
            eng.synthesize(t3.ids, t3.scales, sid=t3.sid)
        else:
            eng.synthesize_batch(big, (0.667, 0.3, 0.8))

    S.pool_scenario(eng, lambda: P.emu_texts(cfg, True), P.join, 3, 48, K.CHUNK, T, CEIL, None, RAMP, between)
    eng.close()


def test_other_modes_are_what_they_were_after_a_detour():
    """Modes 0 to 2 give the same int16, reports and launches before and after the handle has streamed in mode 3."""
    cfg, eng = _engine(own=True)
    ids, nw, nz = K.inputs(cfg)

    def three():
        out = []
        for mode, peak, ramp in (("chunk", 0.0, 0.0), ("running", 0.05, 4.0), ("fixed", 0.5, 0.0)):
            eng.set_stream_gain(mode, peak, ramp)
            eng.profile_enable(2)
            eng.profile_reset()
            per, rep, _ = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
            rows = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
            eng.profile_enable(0)
            out.append((per, rep, rows))
        return out

    before = three()
    assert not any("stream_loudness" in n for _, _, rows in before for n in rows)
    eng.set_stream_loudness(T, CEIL, -30.0, 2.0)
    eng.profile_enable(2)
    eng.profile_reset()
    per3 = S.drain_batch(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    rows3 = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
    eng.profile_enable(0)
    ncalls = len(per3[0])
    # two more graph nodes per chunk than the default mode: the two kernels in stream_gain_kernel's place, the gain conversion
    assert rows3.get("stream_loudness_seg_kernel") == rows3.get("stream_loudness_gain_kernel") == ncalls, rows3
    assert rows3.get("chunk_pcm_gain_kernel") == rows3.get("chunk_peak_kernel") == ncalls and "stream_gain_kernel" not in rows3, rows3
    assert sum(rows3.values()) == sum(before[0][2].values()) + 2 * ncalls, (rows3, before[0][2])
    after = three()
    for (per, rep, rows), (per1, rep1, rows1) in zip(before, after):
        assert rows == rows1
        for b in range(len(ids)):
            assert len(per[b]) == len(per1[b])
            for (a, p), (a1, p1) in zip(per[b], per1[b]):
                assert np.array_equal(a, a1) and np.array_equal(p, p1), b
            assert [tuple(map(float, r)) for r in rep[b]] == [tuple(map(float, r)) for r in rep1[b]], b
    eng.close()


# ---- 5. settings
def test_refusals_and_data_settings():
    cfg, eng = _engine(own=True)
    ids, nw, nz = K.inputs(cfg)
    lib, h = eng._lib, eng._h
    nan = float("nan")
    eng.set_stream_gain("running", 0.05, 4.0)
    gain = eng.stream_gain
    assert eng.stream_loudness[0] is False

    def fails(rc, text, setting, loud):
        assert rc != 0 and text in lib.pe_last_error().decode(), lib.pe_last_error()
        assert eng.stream_gain == setting and eng.stream_loudness == loud

    def refused(setting, loud):
        for bad, text in ((-40.5, "target loudness -40.5"), (-4.0, "target loudness -4"), (nan, "target loudness nan"),
                          (float("inf"), "target loudness inf")):
            fails(lib.pe_set_stream_loudness(h, bad, -1.0, nan, 0), text, setting, loud)
        for bad, text in ((0.5, "peak ceiling 0.5"), (-21.0, "peak ceiling -21"), (nan, "peak ceiling nan")):
            fails(lib.pe_set_stream_loudness(h, -20.0, bad, nan, 0), text, setting, loud)
        for bad, text in ((-71.0, "prior loudness -71"), (1.0, "prior loudness 1"), (float("-inf"), "prior loudness -inf")):
            fails(lib.pe_set_stream_loudness(h, -20.0, -1.0, bad, 0), text, setting, loud)
        for bad in (-1, 65537):
            fails(lib.pe_set_stream_loudness(h, -20.0, -1.0, nan, bad), f"ramp_samples {bad} outside", setting, loud)

    refused(gain, eng.stream_loudness)
    eng.set_stream_loudness(-18.0, -2.0, -25.0, 3.0)
    fs = eng.output_rate
    loud = eng.stream_loudness
    assert loud == (True, -18.0, -2.0, -25.0, round(3.0 * fs / 1000.0)) and eng.stream_gain[0] == "loudness"
    refused(eng.stream_gain, loud)
    # no change while a stream is live: a batch stream, a one-utterance stream (the pool: the pool scenario)
    gen = eng.stream_batch(ids, K.SCALES, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)
    next(gen)
    fails(lib.pe_set_stream_loudness(h, -20.0, -1.0, nan, 0), "cannot change while a stream is live", eng.stream_gain, loud)
    fails(lib.pe_set_stream_gain(h, 0, 0.0, 0), "cannot change while a stream is live", eng.stream_gain, loud)
    gen.close()
    gen = eng.stream(ids[2], tuple(K.SCALES[2]), chunk_frames=K.CHUNK, noise_w=nw[2], noise_z=nz[2])
    next(gen)
    fails(lib.pe_set_stream_loudness(h, -20.0, -1.0, nan, 0), "cannot change while a stream is live", eng.stream_gain, loud)
    for _ in gen:                                          # (to its end: an unfinished stream holds the setting)
        pass
    # pe_set_stream_gain with one of the other modes leaves the mode; the numbers stay readable
    eng.set_stream_gain("chunk")
    assert eng.stream_gain[0] == "chunk" and eng.stream_loudness[:4] == (False,) + loud[1:4]      # (the ramp is the gain's too)
    with pytest.raises(EngineError, match="not set"):
        eng.stream_last_loudness()
    # target, ceiling, prior and ramp are data: once every chunk shape has been seen, new values capture nothing
    eng.set_stream_loudness(-18.0, -2.0, -25.0, 3.0)
    first = S.drain_batch(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    c0 = eng.graph_stats[1]
    eng.set_stream_loudness(-27.0, -6.0, None, 9.0)
    second = S.drain_batch(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    assert eng.graph_stats[1] == c0, (c0, eng.graph_stats)
    S.check_streams(second, fs, -27.0, -6.0, None, round(9.0 * fs / 1000.0), "new values")
    assert any(a.size and not np.array_equal(p, p1) for (a, p, _), (_, p1, _) in zip(first[2], second[2]))
    eng.close()
    # a voice without a header rate has to be told its rate first
    onnx = Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), device=0)
    with pytest.raises(EngineError, match="carries none"):
        onnx.set_stream_loudness(-20.0)
    assert onnx.stream_gain[0] == "chunk"
    onnx.set_output_rate(None, native=16000)
    onnx.set_stream_loudness(-20.0)
    assert onnx.stream_loudness == (True, -20.0, -1.0, None, 80)
    onnx.close()
    with pytest.raises(EngineError, match="7000"):
        tiny_rate = _engine(own=True)[1]
        try:
            tiny_rate.debug_stream_loudness([np.zeros(8, np.float32)], 7000, [[8]])
        finally:
            tiny_rate.close()
