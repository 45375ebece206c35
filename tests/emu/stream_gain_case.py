"""The stream-wide int16 levels (pe_set_stream_gain, include/piper_hip.h) restated in float32 numpy, shared by
tests/test_stream_gain_emu.py and tests/test_gpu_stream_gain.py. The restatement is applied to the floats the engine itself
delivers, the way the existing stream tests apply oracle.audio_float_to_int16: what is under test is the rule, its state
and where the state lives, not the waveform. The inputs are those of stream_batch_case.py."""
import numpy as np

F32 = np.float32
FLOOR = F32(0.01)
FULL = F32(32767.0)
MODES = ("chunk", "running", "fixed")


class Level:
    """One stream's level: a one-utterance stream, a batch-stream row, or a pool slot from join to its end."""

    def __init__(self, mode, peak=0.0, ramp=0):
        assert mode in MODES
        self.mode, self.P, self.R0 = mode, F32(peak), int(ramp)
        self.r = max(FLOOR, self.P)                      # the running peak at begin / join
        self.first = True                                # nothing delivered yet

    def chunk(self, x):
        """(int16 chunk, boolean mask of the ramp's samples, end-of-chunk gain g1, the level it came from) for the floats
        x of the stream's next chunk. x.size == 0 moves nothing."""
        x = np.asarray(x, F32)
        n = x.size
        if n == 0:
            if self.mode == "running":
                return x.astype(np.int16), np.zeros(0, bool), FULL / self.r, self.r
            return x.astype(np.int16), np.zeros(0, bool), F32(0), F32(0)
        c = F32(np.max(np.abs(x)))
        R = 0
        if self.mode == "chunk":
            level = max(FLOOR, c)
            g0 = g1 = FULL / level
        elif self.mode == "fixed":
            level = max(FLOOR, self.P)
            g0 = g1 = FULL / level
        else:
            level = max(self.r, c)
            g1 = FULL / level
            g0 = g1 if self.first else FULL / self.r
            R = min(self.R0, n)
            self.r = level
        self.first = False
        g = np.full(n, g1, F32)
        if R > 0:
            # g(i) = g1 + (g0 - g1) * ((R - 1 - i) / R): an f32 quotient, then ONE fused multiply-add (the product of two
            # floats is exact in f64; the sum is rounded to f64 and then to f32, which differs from the single rounding
            # only in a tie of the second rounding -- and a compiler may contract differently: inside a ramp the int16
            # may differ by one)
            w = (F32(R - 1) - np.arange(R, dtype=F32)) / F32(R)
            d = F32(g0) - F32(g1)
            g[:R] = (np.float64(d) * w.astype(np.float64) + np.float64(g1)).astype(F32)
        pcm = np.clip(x * g, F32(-32768.0), F32(32767.0)).astype(np.int16)
        ramp = np.zeros(n, bool)
        ramp[:R] = True
        return pcm, ramp, F32(g1), F32(level)


def check_chunk(level, x, pcm, where):
    """The engine's int16 chunk against the restatement on the engine's floats: equal outside the ramp, within one inside
    it. Returns (g1, level) of the restatement."""
    want, ramp, g1, lv = level.chunk(x)
    assert pcm.dtype == np.int16 and pcm.shape == want.shape, where
    assert np.array_equal(pcm[~ramp], want[~ramp]), (where, int(np.max(np.abs(pcm[~ramp].astype(int) - want[~ramp]))))
    if ramp.any():
        assert np.max(np.abs(pcm[ramp].astype(np.int32) - want[ramp].astype(np.int32))) <= 1, where
    return g1, lv


def check_stream(chunks, mode, peak=0.0, ramp=0, reports=None, where=""):
    """Every (float, int16) chunk of ONE stream, in order; reports: the (gain, peak) the engine reported after each of them.
    Returns the restated (g1, level) per chunk."""
    lv = Level(mode, peak, ramp)
    out = []
    for k, (a, p) in enumerate(chunks):
        g1, level = check_chunk(lv, a, p, (where, k))
        if reports is not None:
            assert F32(reports[k][0]) == g1 and F32(reports[k][1]) == level, (where, k, reports[k], g1, level)
        out.append((g1, level))
    return out


def pcm_rms(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)) / 32767.0
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def drain(eng, ids, nw, nz, chunk_frames, scales, sids=None):
    """Engine.stream_batch to its end: per utterance the (float, int16) chunks that delivered samples and, aligned with
    them, the (gain, peak) reported for that call; and the full report of every call."""
    B = len(ids)
    per, rep, calls = [[] for _ in ids], [[] for _ in ids], []
    for item in eng.stream_batch(ids, scales, sids=sids, chunk_frames=chunk_frames, noise_w=nw, noise_z=nz):
        g, p = eng.stream_last_gains()
        assert g.shape == p.shape == (B,)
        calls.append((g.copy(), p.copy(), [item[b][1].size for b in range(B)]))
        for b, (a, pc) in enumerate(item):
            if pc.size:
                per[b].append((a, pc))
                rep[b].append((g[b], p[b]))
    return per, rep, calls


def after_peak(chunks):
    """[(chunk index, first sample)] of the chunks behind the one that holds the utterance's peak."""
    pk = [float(np.max(np.abs(a))) for a, _ in chunks]
    kmax = int(np.argmax(pk))
    starts = np.concatenate([[0], np.cumsum([a.size for a, _ in chunks])])
    return [(k, int(starts[k])) for k in range(kmax + 1, len(chunks))]


def check_running_behaviour(per, rep, full_pcm, rms_tol, where):
    """The running mode without prior and ramp, for every utterance: the restatement, the reported peaks as running maxima
    of the chunk peaks, the last one the maximum of everything delivered, gains that never rise, and behind the peak chunk
    the int16 of the whole-utterance call."""
    for b, chunks in enumerate(per):
        got = check_stream(chunks, "running", 0.0, 0, reports=rep[b], where=(where, b))
        pk = np.array([np.max(np.abs(a)) for a, _ in chunks], F32)
        peaks = np.array([r[1] for r in rep[b]], F32)
        gains = np.array([r[0] for r in rep[b]], F32)
        assert np.array_equal(peaks, np.maximum(FLOOR, np.maximum.accumulate(pk))), (where, b)
        assert peaks[-1] == np.max(np.abs(np.concatenate([a for a, _ in chunks]))), (where, b)
        assert np.all(np.diff(gains) <= 0) and np.array_equal(gains, FULL / peaks), (where, b)
        assert [g for g, _ in got] == list(gains)
        for k, s in after_peak(chunks):
            p = chunks[k][1]
            assert pcm_rms(p, full_pcm[b][s:s + p.size]) <= rms_tol, (where, b, k)


def check_ramps(per, rep, ramp, where, prior=0.0, min_active=1):
    """The restatement and the reports, and -- on the engine's own int16 -- the ramp's last sample at exactly g1, also
    where the chunk is shorter than the ramp; where the gain fell, the ramp is really there and never below g1."""
    active = 0
    for b, chunks in enumerate(per):
        check_stream(chunks, "running", prior, ramp, reports=rep[b], where=(where, ramp, b))
        prev = None
        for k, (a, p) in enumerate(chunks):
            g1 = F32(rep[b][k][0])
            R = min(ramp, a.size)
            plain = np.clip(a * g1, F32(-32768.0), F32(32767.0)).astype(np.int16)
            assert p[R - 1] == plain[R - 1], (where, ramp, b, k)
            assert np.array_equal(p[R:], plain[R:]), (where, ramp, b, k)
            if prev is not None and g1 < prev:
                active += 1
                assert not np.array_equal(p[:R], plain[:R]), (where, ramp, b, k)
                assert np.all(np.abs(p[:R].astype(np.int32)) >= np.abs(plain[:R].astype(np.int32))), (where, ramp, b, k)
            prev = g1
    assert active >= min_active, (where, ramp, active)


def check_finished_rows_keep_their_state(rep, calls):
    """A batch-stream row that has finished delivers nothing and keeps reporting the state it ended with."""
    for b in range(len(rep)):
        for g, p, sizes in calls[len(rep[b]):]:
            assert sizes[b] == 0 and (g[b], p[b]) == tuple(rep[b][-1]), b


class Tenant:
    """A pool slot's tenant: the listener, its level's restatement, what it received."""

    def __init__(self, x, slot, prior, ramp):
        self.x, self.slot, self.level = x, slot, Level("running", prior, ramp)
        self.chunks, self.reports = [], []


def pool_step(eng, pool, on, chunk):
    """One pool call: every delivered chunk against ITS slot's level (restatement and report)."""
    out = pool.next(chunk)
    g, p = eng.stream_last_gains()
    assert g.shape == (pool.slots,)
    for s, t in on.items():
        if s not in out:
            continue
        a, pc = out[s]
        g1, lv = check_chunk(t.level, a, pc, ("pool", t.x.name, len(t.chunks)))
        assert (g[s], p[s]) == (g1, lv), (t.x.name, len(t.chunks), g[s], p[s], g1, lv)
        t.chunks.append((a, pc))
        t.reports.append((g1, lv))
    return out


def pool_scenario(eng, make_texts, join, slots, max_frames, chunk, prior, ramp, between, one_tol, rms_tol):
    """The pool in the running mode. make_texts() -> fresh listeners [short, mid, long, fourth]; join(pool, listeners) ->
    slots (tests/stream_pool_case.py); between(k): other calls on the handle between two chunks (k = 0: a whole-utterance
    call, k = 1: one that grows the workspaces). Long and mid stream for two calls, short joins them in mid-stream, a join
    without room fails, short finishes and the fourth text takes its slot, long hangs up and short's text takes that slot;
    every chunk is held to its own slot's level (which slot the fourth text gets depends on who has finished by then: the
    lowest free one, which had a tenant). Then short again, alone in a fresh pool."""
    from piper_amd.engine import EngineError
    t0, t1, t2, t3 = make_texts()
    eng.set_stream_gain("running", prior, ramp * 1000.0 / eng.output_rate)
    assert eng.stream_gain == ("running", F32(prior), ramp)
    pool = eng.stream_pool(slots, max_frames)
    on = {}

    def enter(xs):
        got = join(pool, xs)
        for x, s in zip(xs, got):
            on[s] = Tenant(x, s, prior, ramp)
        return got

    assert enter([t2, t1]) == [0, 1]
    pool_step(eng, pool, on, chunk)
    pool_step(eng, pool, on, chunk)
    assert enter([t0]) == [2]
    between(0)
    pool_step(eng, pool, on, chunk)
    between(1)
    nfree = len(pool.free_slots)
    try:
        join(pool, make_texts()[:nfree + 1])
        raise AssertionError("a join without room succeeded")
    except EngineError as e:
        assert "free slots" in str(e)
    setting = eng.stream_gain
    try:
        eng.set_stream_gain("fixed", 0.5)
        raise AssertionError("the gain changed under an occupied pool")
    except EngineError as e:
        assert "occupied" in str(e) and eng.stream_gain == setting
    pool_step(eng, pool, on, chunk)
    newcomer = on[2]
    assert len(on[0].chunks) == 4 and len(newcomer.chunks) == 2
    # slot 2's tenant finishes; the fourth text takes the slot and starts from the prior, not from that tenant's peak
    while pool.frames_done[2] < t0.frames:
        pool_step(eng, pool, on, chunk)
    free = pool.free_slots
    assert 2 in free and free[0] in on and on[free[0]].reports[-1][1] > F32(prior)      # the lowest free slot had a tenant
    s3 = enter([t3])[0]
    assert s3 == free[0]
    pool_step(eng, pool, on, chunk)
    assert on[s3].reports[0][1] == max(F32(prior), F32(np.max(np.abs(on[s3].chunks[0][0]))))
    # the longest listener hangs up; its slot goes to the short text: that level is its own from the first chunk on
    assert pool.frames_done[0] < t2.frames and on[0].reports[-1][1] > F32(prior)
    pool.leave(0)
    assert enter([make_texts()[0]]) == [0]
    while pool_step(eng, pool, on, chunk):
        pass
    assert on[0].reports[0][1] == max(F32(prior), F32(np.max(np.abs(on[0].chunks[0][0]))))
    assert len(on[0].chunks) == len(newcomer.chunks)
    g, p = eng.stream_last_gains()                       # every finished slot keeps reporting what it ended with
    for s in (0, 1, 2):
        assert (g[s], p[s]) == on[s].reports[-1], s
    pool.close()
    pool = eng.stream_pool(slots, max_frames)
    on = {}
    enter([make_texts()[0]])
    while pool_step(eng, pool, on, chunk):
        pass
    assert len(on[0].chunks) == len(newcomer.chunks)
    for k, ((a, pc), (a1, pc1)) in enumerate(zip(newcomer.chunks, on[0].chunks)):
        assert np.max(np.abs(a - a1)) < one_tol and pcm_rms(pc, pc1) <= rms_tol, k
    pool.close()
    eng.set_stream_gain("chunk")
