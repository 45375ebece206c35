"""One gain across a stream's chunks (pe_set_stream_gain: running-peak and fixed levels beside the default per-chunk rule) on
the test-only emulator build of the engine, the activation workspaces poisoned. The rule is restated in float32 numpy in
tests/emu/stream_gain_case.py and applied to the floats the engine delivers: int16 equal outside ramps, within one inside
them. Inputs: the three texts of tests/emu/stream_batch_case.py (6, 14 and 23 ids, chunks of 4 frames, injected noise).
The GPU counterpart is tests/test_gpu_stream_gain.py (-m gpu)."""
import hashlib
import json
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
import stream_batch_case as K                            # noqa: E402
import stream_gain_case as G                             # noqa: E402
import stream_pool_case as P                             # noqa: E402

ONE_TOL, RMS_TOL = 1e-5, 1e-3                            # tests/test_stream_batch_emu.py, same inputs
F32 = np.float32


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _engine(emu_lib, preset):
    """An engine whose workspaces are poisoned with NaN patterns before use (read at creation)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PIPER_HIP_DEBUG_POISON", "1")
        cfg = W.preset(preset)
        return cfg, Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), lib=emu_lib)


@pytest.fixture(scope="module")
def tiny(emu_lib):
    cfg, eng = _engine(emu_lib, "tiny")
    yield cfg, eng, K.inputs(cfg)
    eng.close()


@pytest.fixture(scope="module")
def default_run(tiny):
    """The ragged stream in the default mode -- after a detour through the running mode -- with per-launch profiling on."""
    cfg, eng, (ids, nw, nz) = tiny
    eng.set_stream_gain("running", 0.3, 2.0)
    eng.set_stream_gain("chunk")
    assert eng.stream_gain[0] == "chunk"
    eng.profile_enable(2)
    eng.profile_reset()
    per, rep, calls = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    rows = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
    eng.profile_enable(0)
    return per, rep, calls, rows


@pytest.fixture(scope="module")
def running_run(tiny):
    """The same stream in the running mode without a prior and without a ramp, and the whole-utterance call."""
    cfg, eng, (ids, nw, nz) = tiny
    eng.set_stream_gain("running", 0.0, 0.0)
    assert eng.stream_gain == ("running", 0.0, 0)
    per, rep, calls = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    full = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    eng.set_stream_gain("chunk")
    return per, rep, calls, full


def _peaks(chunks):
    return [float(np.max(np.abs(a))) for a, _ in chunks]


# ---- 1. the input does what the feature is for
def test_precondition_quiet_chunks_follow_the_peak(default_run):
    per = default_run[0]
    pk = _peaks(per[2])
    kmax = int(np.argmax(pk))
    quiet = [p for p in pk[kmax + 1:] if p < 0.9 * pk[kmax]]
    print("\nutterance 2 chunk peaks", [round(p, 3) for p in pk])
    assert len(per[2]) == 11 and len(quiet) >= 3, pk


# ---- 2. + 3. running mode without a ramp, and what the default mode does on the same chunks
def test_running_level_is_the_whole_utterances_behind_the_peak(default_run, running_run):
    per, rep, calls, full = running_run
    assert [len(c) for c in per] == [len(c) for c in default_run[0]]
    for b in range(3):                                     # the floats do not depend on the mode
        for (a, _), (a0, _) in zip(per[b], default_run[0][b]):
            assert np.array_equal(a, a0), b
    G.check_running_behaviour(per, rep, full.pcm, RMS_TOL, "native")
    assert len(G.after_peak(per[2])) >= 5


def test_default_mode_misses_that_gate_on_the_same_chunks(default_run, running_run):
    """Without the feature: the same chunks, every one normalised by its own peak, are NOT the whole utterance's samples."""
    per0, full = default_run[0], running_run[3]
    pk = _peaks(per0[2])
    missed = 0
    for k, s in G.after_peak(per0[2]):
        p = per0[2][k][1]
        assert np.array_equal(p, G.Level("chunk").chunk(per0[2][k][0])[0])
        if pk[k] < 0.9 * max(pk):
            assert G.pcm_rms(p, full.pcm[2][s:s + p.size]) > RMS_TOL, k
            missed += 1
    assert missed >= 3


# ---- 4. ramps
@pytest.mark.parametrize("ramp", [64, 3000])
def test_ramps(tiny, ramp):
    cfg, eng, (ids, nw, nz) = tiny
    eng.set_stream_gain("running", 0.0, ramp * 1000.0 / eng.output_rate)
    assert eng.stream_gain == ("running", 0.0, ramp)
    per, rep, _ = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    eng.set_stream_gain("chunk")
    assert ramp < per[2][0][0].size or ramp > per[2][0][0].size + 1000          # inside a chunk / longer than one
    G.check_ramps(per, rep, ramp, "native", min_active=3)


# ---- 5. a prior, and a fixed level
def test_prior_and_fixed(tiny):
    cfg, eng, (ids, nw, nz) = tiny
    eng.set_stream_gain("running", 0.5, 0.0)
    per, rep, _ = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    for b in range(3):
        G.check_stream(per[b], "running", 0.5, 0, reports=rep[b], where=("prior", b))
    assert rep[0][-1][1] == F32(0.5) and rep[2][-1][1] > F32(0.5)          # a prior above / below the utterance's peak
    eng.set_stream_gain("fixed", 0.5)
    assert eng.stream_gain[:2] == ("fixed", 0.5)
    per4, rep4, calls4 = G.drain(eng, ids, nw, nz, 4, K.SCALES)
    per7, rep7, _ = G.drain(eng, ids, nw, nz, 7, K.SCALES)
    g = F32(32767.0) / F32(0.5)
    for b in range(3):
        for per_, rep_ in ((per4, rep4), (per7, rep7)):
            G.check_stream(per_[b], "fixed", 0.5, 0, reports=rep_[b], where=("fixed", b))
            assert all(r == (g, F32(0.5)) for r in rep_[b])
        a4, a7 = (np.concatenate([a for a, _ in x[b]]) for x in (per4, per7))
        p4, p7 = (np.concatenate([p for _, p in x[b]]) for x in (per4, per7))
        # one level whatever the chunking: the int16 differs only where the floats of the two chunkings do (they are held
        # to 1e-5 of the unchunked waveform; times 65534 that is under one step)
        assert a4.shape == a7.shape and np.max(np.abs(a4 - a7)) < 2 * ONE_TOL
        same = a4 == a7
        print(f"\nfixed, utterance {b}: {int(same.sum())} of {same.size} floats equal between chunks of 4 and 7 frames")
        assert np.array_equal(p4[same], p7[same]) and np.max(np.abs(p4.astype(np.int32) - p7)) <= 2
    # rows that deliver nothing report 0 in the fixed mode
    assert calls4[-1][2][0] == 0 and calls4[-1][0][0] == 0 and calls4[-1][1][0] == 0
    # the one-utterance stream, which converts on the host: the same rule
    one = list(eng.stream(ids[1], tuple(K.SCALES[1]), chunk_frames=7, noise_w=nw[1], noise_z=nz[1]))
    G.check_stream(one, "fixed", 0.5, 0, where="fixed, one utterance")
    assert eng.stream_last_gains()[0][0] == 0                                  # (the call that ended it delivered nothing)
    eng.set_stream_gain("chunk")


# ---- 6. ragged batch on the multi-speaker voice, against the one-utterance stream
def test_ragged_batch_and_the_one_utterance_stream(emu_lib):
    cfg, eng = _engine(emu_lib, "tiny-ms")
    ids, nw, nz = K.inputs(cfg)
    sids = list(K.SIDS)
    ramp, prior = 64, 0.05
    eng.set_stream_gain("running", prior, ramp * 1000.0 / eng.output_rate)
    assert eng.stream_gain == ("running", F32(prior), ramp)
    per, rep, calls = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES_MS, sids=sids)
    nchunks = [len(c) for c in per]
    assert min(nchunks) + 3 <= max(nchunks), nchunks
    # a finished utterance delivers nothing and keeps reporting the state it ended with
    G.check_finished_rows_keep_their_state(rep, calls)
    for b in range(3):
        G.check_stream(per[b], "running", prior, ramp, reports=rep[b], where=("batch", b))
        one, rep1 = [], []
        for a, p in eng.stream(ids[b], tuple(float(v) for v in K.SCALES_MS[b]), sid=sids[b], chunk_frames=K.CHUNK,
                               noise_w=nw[b], noise_z=nz[b]):
            one.append((a, p))
            g1, p1 = eng.stream_last_gains()
            assert g1.shape == (1,)
            rep1.append((g1[0], p1[0]))
        assert len(one) == len(per[b]), b
        G.check_stream(one, "running", prior, ramp, reports=rep1, where=("one", b))
        assert tuple(eng.stream_last_gains()[i][0] for i in (0, 1)) == rep1[-1]          # the stored state, nothing delivered
        for k, ((a, p), (a1, p1)) in enumerate(zip(per[b], one)):
            assert a.shape == a1.shape and np.max(np.abs(a - a1)) < ONE_TOL, (b, k)
            assert G.pcm_rms(p, p1) <= RMS_TOL, (b, k)
    eng.close()


# ---- 7. the pool: one level per slot, resident, reset by the join
def test_pool_levels_are_per_slot_and_resident(emu_lib):
    """Three slots on the multi-speaker voice (tests/emu/stream_gain_case.py: pool_scenario): a newcomer joins two residents in
    mid-stream; a whole-utterance call, a batch that grows both workspaces (and poisons them again) and a join without room
    happen between two chunks; a finished tenant's slot and a departed listener's slot are reused. Every chunk is held to
    its own slot's level, and a new tenant starts from the prior."""
    cfg, eng = _engine(emu_lib, "tiny-ms")
    big = [W.synthetic_phoneme_ids(T, 90 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate((136, 3, 4, 5))]
    t3 = P.emu_texts(cfg, True)[3]

    def between(k):
        if k == 0:
            eng.synthesize(t3.ids, t3.scales, sid=t3.sid)
        else:
            eng.synthesize_batch(big, (0.667, 0.3, 0.8))

    G.pool_scenario(eng, lambda: P.emu_texts(cfg, True), P.join, 3, 48, K.CHUNK, 0.05, 64, between, ONE_TOL, RMS_TOL)
    eng.close()


# ---- 8. with an output rate set: the resampled twin, peaks and ramps in output samples
@pytest.mark.parametrize("rate", [8000, 48000])
def test_with_an_output_rate(emu_lib, rate):
    cfg, eng = _engine(emu_lib, "tiny")
    ids, nw, nz = K.inputs(cfg)
    eng.set_output_rate(rate)
    eng.set_stream_gain("running", 0.0, 0.0)
    per, rep, _ = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
    full = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    n0 = per[2][0][0].size
    assert n0 == -(-K.CHUNK * eng.hop * rate // cfg.sample_rate)
    G.check_running_behaviour(per, rep, full.pcm, RMS_TOL, rate)
    for ramp in (64, 3000):
        eng.set_stream_gain("running", 0.0, ramp * 1000.0 / rate)
        assert eng.stream_gain == ("running", 0.0, ramp)
        per, rep, _ = G.drain(eng, ids, nw, nz, K.CHUNK, K.SCALES)
        G.check_ramps(per, rep, ramp, rate, min_active=3)
    eng.close()


# ---- 9. errors change nothing
def test_errors_change_nothing(emu_lib):
    cfg, eng = _engine(emu_lib, "tiny-ms")
    ids, nw, nz = K.inputs(cfg)
    sids = list(K.SIDS)
    lib, h = emu_lib, eng._h
    eng.set_stream_gain("running", 0.05, 4.0)
    setting = eng.stream_gain
    ramp = setting[2]
    assert ramp == round(4.0 * eng.output_rate / 1000.0)

    def fails(rc, text):
        assert rc != 0 and text in lib.pe_last_error().decode(), lib.pe_last_error()
        assert eng.stream_gain == setting

    def refused():
        fails(lib.pe_set_stream_gain(h, 3, 0.1, 0), "unknown stream gain mode")
        fails(lib.pe_set_stream_gain(h, -1, 0.1, 0), "unknown stream gain mode")
        fails(lib.pe_set_stream_gain(h, 1, float("nan"), 0), "peak is not finite")
        fails(lib.pe_set_stream_gain(h, 2, float("inf"), 0), "peak is not finite")
        fails(lib.pe_set_stream_gain(h, 1, -0.1, 0), "peak must not be negative")
        fails(lib.pe_set_stream_gain(h, 2, 0.0, 0), "needs a peak > 0")
        fails(lib.pe_set_stream_gain(h, 1, 0.1, -1), "ramp_samples outside")
        fails(lib.pe_set_stream_gain(h, 1, 0.1, 65537), "ramp_samples outside")

    refused()
    with pytest.raises(ValueError):
        eng.set_stream_gain("agc")
    eng.set_stream_gain("running", 0.05, 65536 * 1000.0 / eng.output_rate)      # the largest ramp is accepted
    assert eng.stream_gain[2] == 65536
    eng.set_stream_gain(*setting[:2], ramp_ms=4.0)
    assert eng.stream_gain == setting
    # while a batch stream is live: every valid change is refused by name too, and the next chunk is what it would have been
    gen = eng.stream_batch(ids, K.SCALES_MS, sids=sids, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)
    levels = [G.Level("running", 0.05, ramp) for _ in ids]
    first = next(gen)
    refused()
    for mode in (0, 1, 2):
        fails(lib.pe_set_stream_gain(h, mode, 0.5, 0), "cannot change while a stream is live")
    second = next(gen)
    for item in (first, second):
        for b, (a, p) in enumerate(item):
            G.check_chunk(levels[b], a, p, ("batch", b))
    gen.close()
    # ... a one-utterance stream
    gen = eng.stream(ids[2], tuple(float(v) for v in K.SCALES_MS[2]), sid=sids[2], chunk_frames=K.CHUNK, noise_w=nw[2], noise_z=nz[2])
    lv = G.Level("running", 0.05, ramp)
    a, p = next(gen)
    fails(lib.pe_set_stream_gain(h, 0, 0.0, 0), "cannot change while a stream is live")
    a1, p1 = next(gen)
    G.check_chunk(lv, a, p, "one 0")
    G.check_chunk(lv, a1, p1, "one 1")
    gen.close()
    # ... (that stream is still unfinished: ended by the next upload) and a pool with an occupied slot
    texts = P.emu_texts(cfg, True)
    with eng.stream_pool(2, 48) as pool:
        P.join(pool, [texts[1]])
        lv = G.Level("running", 0.05, ramp)
        out = pool.next(K.CHUNK)
        fails(lib.pe_set_stream_gain(h, 2, 0.5, 0), "cannot change while a stream pool slot is occupied")
        out1 = pool.next(K.CHUNK)
        G.check_chunk(lv, *out[0], "pool 0")
        G.check_chunk(lv, *out1[0], "pool 1")
        pool.leave(0)
        eng.set_stream_gain("fixed", 0.25, 0.0)                                 # an open pool without tenants does not hold it
        assert eng.stream_gain == ("fixed", 0.25, 0)
    eng.close()


# ---- 10. the default is what it was
def test_default_mode_is_untouched(default_run):
    per, rep, calls, rows = default_run
    ncalls = len(calls)
    assert rows.get("window_gather_kernel") == rows.get("chunk_peak_kernel") == rows.get("chunk_pcm_kernel") == ncalls, rows
    assert not [n for n in rows if "_gain_" in n], rows
    for b in range(3):
        G.check_stream(per[b], "chunk", reports=rep[b], where=("default", b))
    h = hashlib.sha256()
    for chunks in per:
        for _, p in chunks:
            h.update(np.ascontiguousarray(p).tobytes())
    child = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu", "stream_batch_case.py")], capture_output=True,
                           text=True, timeout=900)
    assert child.returncode == 0, child.stderr[-2000:]
    want = json.loads(child.stdout.strip().splitlines()[-1])
    assert want["chunks"] == [len(c) for c in per] and want["pcm_sha256"] == h.hexdigest()
