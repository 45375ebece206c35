"""Streams at a target loudness (pe_set_stream_loudness, kernels/stream_loudness.h): the f64 restatement of DESIGN.md 4.9 and
the cases shared by tests/test_stream_loudness_emu.py and tests/test_gpu_stream_loudness.py. It builds on
tests/loudness_case.py -- the serial f64 K-weighting, the blocks and gates, the tolerances -- and looks at no kernel: the
running loudness of a prefix is the whole-utterance loudness of that prefix, the rule is written out in Python floats, and
the int16 is formed from the floats the engine delivers with the gains the engine reports."""
import math

import numpy as np

import loudness_case as LC
from loudness_case import SHORT, UNMEASURABLE, LIMITED, L_TOL, SCALE_TOL, GATE_MARGIN, Truth

PRIOR = 16
F32 = np.float32
EMPTY = (-math.inf, 0.0, 0.0, SHORT | UNMEASURABLE)      # the report of a stream that has delivered nothing yet
MAX_EXCLUDED = 0.1                                       # chunks per test whose prefix has a block within GATE_MARGIN of a gate


class Prefix(Truth):
    """Truth of the prefix X[0 .. N) of a row whose K-weighted squares y2 are known: the filter is causal, so the prefix's
    y^2 are the row's. Everything else is Truth's arithmetic, by calling it on the cut row with the filter swapped out."""

    def __init__(self, x, y2, N, fs):
        keep = LC.kweight_sq
        LC.kweight_sq = lambda xs, f: y2[:N]
        try:
            Truth.__init__(self, np.asarray(x, F32)[:N], fs)
        finally:
            LC.kweight_sq = keep


def rule(t, T, ceiling_db, prior, r_new, G, first, lu):
    """Steps 2 to 6 of the contract in f64 for a chunk whose prefix has the truth t: (g0, g1, flags, lu')."""
    ok = not t.flags & UNMEASURABLE
    short = bool(t.flags & SHORT)
    flags = t.flags & (SHORT | UNMEASURABLE)
    Lu = None
    if ok and not (short and prior is not None):
        Lu = t.L
    elif prior is not None:
        Lu, flags = float(prior), flags | PRIOR
    elif lu is not None:
        Lu = lu
    a = 10.0 ** ((T - Lu) / 20.0) if Lu is not None else 1.0
    cap = cap_of(ceiling_db, r_new)
    g1 = 32767.0 * a
    if cap < g1:
        g1, flags = cap, flags | LIMITED
    g0 = g1 if first else min(G, cap)
    return g0, g1, flags, (Lu if Lu is not None else lu)


def cap_of(ceiling_db, r_new):
    """(float)(32767 C / r'), one ulp less where the rounding would lift r' over the ceiling; C travels as an f32."""
    if not r_new > 0:
        return math.inf
    lim = 32767.0 * float(F32(10.0 ** (ceiling_db / 20.0)))
    cap = F32(lim / float(r_new))
    if float(cap) * float(r_new) > lim:
        cap = np.nextafter(cap, F32(0))
    return float(cap)


def convert(x, g0, g1, R):
    """chunk_pcm_gain_kernel's arithmetic (tests/emu/stream_gain_case.py): (int16, mask of the ramp)."""
    x = np.asarray(x, F32)
    g = np.full(x.size, F32(g1), F32)
    if R > 0:
        w = (F32(R - 1) - np.arange(R, dtype=F32)) / F32(R)
        d = F32(g0) - F32(g1)
        g[:R] = (np.float64(d) * w.astype(np.float64) + np.float64(F32(g1))).astype(F32)
    ramp = np.zeros(x.size, bool)
    ramp[:R] = True
    return np.clip(x * g, F32(-32768.0), F32(32767.0)).astype(np.int16), ramp


class Stream:
    """One stream's restatement: fed the floats of every chunk and what the engine reported for it."""

    def __init__(self, fs, T, ceiling_db, prior, R0, y2=None, row=None):
        self.fs, self.T, self.cdb, self.prior, self.R0 = fs, T, ceiling_db, prior, int(R0)
        self.X = np.zeros(0, F32)
        self.r, self.G, self.lu, self.first = F32(0), None, None, True
        self.y2, self.row = y2, row
        self.last = EMPTY
        self.checked = self.excluded = 0
        self.trace = []                                  # (N, truth L, reported L, truth g1, reported g1, flags)

    def chunk(self, x, pcm, report, where, g0_dev=None, last=False):
        """x: the chunk's floats, pcm its int16, report = (L, g1, peak, flags) the engine gave for the stream after it."""
        x = np.asarray(x, F32)
        if x.size == 0:
            assert tuple_eq(report, self.last), (where, report, self.last)
            return
        self.X = np.concatenate([self.X, x])
        N = self.X.size
        t = Prefix(self.row, self.y2, N, self.fs) if self.y2 is not None else Truth(self.X, self.fs)
        r_new = max(self.r, F32(np.max(np.abs(x))))
        g0, g1, flags, lu = rule(t, self.T, self.cdb, self.prior, r_new, self.G, self.first, self.lu)
        L, dg1, peak, dflags = float(report[0]), float(report[1]), F32(report[2]), int(report[3])
        self.trace.append((N, t.L, L, g1, dg1, dflags))
        assert peak == r_new, (where, peak, r_new)
        near_gate = t.margin < GATE_MARGIN
        assert not (near_gate and last), (where, "the stream's last prefix lies within the gate margin", t.margin)
        self.checked += 1
        if near_gate:
            self.excluded += 1                           # a block may flip by rounding: L, gain and flags follow it
        else:
            assert dflags == flags, (where, N, dflags, flags)
            if flags & UNMEASURABLE:
                assert L == -math.inf, (where, L)
            else:
                assert abs(L - t.L) <= L_TOL, (where, N, L, t.L)
            assert abs(dg1 - g1) <= SCALE_TOL * g1, (where, N, dg1, g1)
        # the conversion, with the gains the device used: g1 as reported, g0 by the rule from the reported numbers
        cap = cap_of(self.cdb, r_new)
        dg0 = dg1 if self.first else min(float(self.G_dev), cap)
        if g0_dev is not None:
            assert F32(g0_dev) == F32(dg0), (where, N, g0_dev, dg0)
        if not near_gate:
            assert abs(dg0 - g0) <= SCALE_TOL * g0, (where, N, dg0, g0)
        assert dg1 <= cap and dg0 <= cap, (where, dg0, dg1, cap)
        R = min(self.R0, x.size)
        want, ramp = convert(x, dg0, dg1, R)
        assert pcm.dtype == np.int16 and pcm.shape == want.shape, where
        assert np.array_equal(pcm[~ramp], want[~ramp]), (where, N)
        if ramp.any():
            assert np.max(np.abs(pcm[ramp].astype(np.int32) - want[ramp].astype(np.int32))) <= 1, (where, N)
        # the ceiling holds on every delivered sample
        top = math.floor(32767.0 * float(F32(10.0 ** (self.cdb / 20.0))))
        a = np.abs(pcm.astype(np.int32))
        assert (a[~ramp].max() if (~ramp).any() else 0) <= top and (a[ramp].max() if ramp.any() else 0) <= top + 1, (where, N, int(a.max()), top)
        self.r, self.G, self.G_dev, self.lu, self.first = r_new, g1, F32(dg1), lu, False
        self.last = (L, dg1, float(peak), dflags)


def tuple_eq(a, b):
    return all((float(u) == float(v)) or (u != u and v != v) for u, v in zip(a, b)) and int(a[3]) == int(b[3])


def assert_exclusions(streams, where):
    checked = sum(s.checked for s in streams)
    excluded = sum(s.excluded for s in streams)
    print(f"{where}: {checked} chunks checked, {excluded} within the gate margin")
    assert checked > 0 and excluded <= MAX_EXCLUDED * checked, (where, excluded, checked)


# ---- 1. kernel rows through the debug entry --------------------------------------------------------------------------
def chunkings(n, fs):
    """Three ways to cut a row of n samples: one chunk; the state's corner cases in a row; many odd chunks."""
    h, W = (fs + 5) // 10, (fs + 10) // 20
    one = [n]
    corner, done = [], 0

    def take(c):
        nonlocal done
        c = max(0, min(c, n - done))
        corner.append(c)
        done += c

    for c in (W // 3, W // 3, W // 3 - 1, 1, 0):          # shorter than W, several in a row; one sample; an empty one
        take(c)
    take(h - done % h if done % h else 0)                # ... up to a segment boundary exactly
    take(h)                                              # boundary to boundary
    take(h // 2)                                         # a boundary inside a segment
    take(3 * h + 17)                                     # three segments and more
    take(0)
    take(2 * h - (h // 2 + 17))                          # back on a segment boundary
    take(W - 1)
    take(n)                                              # the rest
    step = (3 * h) // 7 + 1
    odd = [step] * (n // step) + ([n % step] if n % step else [])
    return [one, corner, odd or [0]]


def check_kernel(eng, fs, T=-23.0, ceiling_db=-1.0, ramp=96):
    """Every row of loudness_case.kernel_rows(fs), each cut three ways over three calls in which neighbouring rows are cut
    differently: every L_k against the f64 truth of the prefix, the final L against Truth of the whole row, the chunkings
    against each other. Returns the streams."""
    rows = LC.kernel_rows(fs)
    y2 = [LC.kweight_sq(x, fs) for _, x in rows]
    whole = [Truth(x, fs) for _, x in rows]
    for t, (name, _) in zip(whole, rows):
        assert t.margin >= GATE_MARGIN, (fs, name, t.margin)
    cuts = [chunkings(x.size, fs) for _, x in rows]
    finals = [[] for _ in rows]
    streams = []
    for call in range(3):
        pick = [cuts[b][(b + call) % 3] for b in range(len(rows))]
        K = max(len(c) for c in pick)
        table = np.zeros((K, len(rows)), np.int32)
        for b, c in enumerate(pick):
            table[:len(c), b] = c
        L, g0, g1, flags, pcm = eng.debug_stream_loudness([x for _, x in rows], fs, table, T, ceiling_db, None, ramp)
        for b, (name, x) in enumerate(rows):
            s = Stream(fs, T, ceiling_db, None, ramp, y2=y2[b], row=x)
            streams.append(s)
            done, lastk = 0, max([k for k in range(K) if table[k, b] > 0], default=-1)
            for k in range(K):
                c = int(table[k, b])
                peak = max(s.r, F32(np.max(np.abs(x[done:done + c])))) if c else s.last[2]
                s.chunk(x[done:done + c], pcm[b][done:done + c], (L[k, b], g1[k, b], peak, flags[k, b]),
                        (fs, name, call, k), g0_dev=g0[k, b] if c else None, last=k == lastk)
                done += c
            assert done == x.size
            if x.size:
                t = whole[b]
                assert s.last[3] & (SHORT | UNMEASURABLE) == t.flags, (fs, name, call)
                if not t.flags & UNMEASURABLE:
                    assert abs(s.last[0] - t.L) <= L_TOL, (fs, name, call, s.last[0], t.L)
                    finals[b].append(s.last[0])
    for b, (name, _) in enumerate(rows):
        if finals[b]:
            assert len(finals[b]) == 3 and max(finals[b]) - min(finals[b]) <= L_TOL, (fs, name, finals[b])
            print(f"{fs} Hz, {name}: final L by three chunkings {['%.6f' % v for v in finals[b]]} (f64 {whole[b].L:.6f})")
    # what the cases are for: a SHORT -> block transition, gated blocks, chunks below W and across three segments
    h = (fs + 5) // 10
    long_s = [s for s in streams if s.row is not None and s.row.size == 13 * h + 7]
    assert any(any(f & SHORT for *_, f in s.trace) and not s.trace[-1][5] & SHORT for s in long_s)
    assert_exclusions(streams, f"kernel rows at {fs} Hz")
    return streams


# ---- 2. the rule ---------------------------------------------------------------------------------------------------
def tone(n, fs, amp, f=440.0):
    return (amp * np.sin(2 * np.pi * f * np.arange(n, dtype=np.float64) / fs)).astype(F32)


def rule_rows(fs):
    """Rows whose chunks walk the rule's branches at rate fs: (name, row, chunk lengths, prior, what must show)."""
    h = (fs + 5) // 10
    quiet_then_tone = np.concatenate([np.zeros(2 * h, F32), tone(6 * h, fs, 0.05)])
    click_late = tone(8 * h, fs, 0.02)
    click_late[5 * h + 10] = 0.9                         # one sample: the loudness stays, the peak does not
    return [
        # silence first: unmeasurable -> the prior; then SHORT with a prior -> still the prior; then blocks -> L_k
        ("prior", quiet_then_tone, [2 * h, h, h, 2 * h, 2 * h], -36.0),
        # no prior, a silent first chunk: a = 1 (delivered as generated), then the measured gain comes in over the ramp
        ("silent-first", quiet_then_tone, [2 * h, h, h, 2 * h, 2 * h], None),
        # a soft stream whose target gain is far above what its late peak allows: LIMITED, g0 cut to the new cap
        ("late-peak", click_late, [2 * h, 2 * h, h + h // 3, h, 2 * h - h // 3], None),
    ]


def check_rule(eng, fs, T=-16.0, ceiling_db=-3.0):
    out = {}
    for ramp in (0, 64, 65536):                        # no ramp; inside a chunk; larger than every chunk
        for name, x, cuts, prior in rule_rows(fs):
            table = np.asarray(cuts, np.int32).reshape(-1, 1)
            L, g0, g1, flags, pcm = eng.debug_stream_loudness([x], fs, table, T, ceiling_db, prior, ramp)
            s = Stream(fs, T, ceiling_db, prior, ramp)
            done = 0
            for k, c in enumerate(cuts):
                peak = max(s.r, F32(np.max(np.abs(x[done:done + c]))))
                s.chunk(x[done:done + c], pcm[0][done:done + c], (L[k, 0], g1[k, 0], peak, flags[k, 0]), (fs, name, ramp, k),
                        g0_dev=g0[k, 0], last=k == len(cuts) - 1)
                done += c
            assert s.excluded == 0, (name, ramp)
            out[(name, ramp)] = (s, L[:, 0], g0[:, 0], g1[:, 0], flags[:, 0], pcm[0], x, cuts)
    for ramp in (0, 64, 65536):
        s, L, g0, g1, flags, pcm, x, cuts = out[("prior", ramp)]
        a_prior = F32(32767.0 * 10.0 ** ((T + 36.0) / 20.0))
        assert flags[0] == SHORT | UNMEASURABLE | PRIOR and flags[1] == SHORT | PRIOR and not flags[-1] & (PRIOR | SHORT), flags
        assert abs(g1[0] - a_prior) <= SCALE_TOL * a_prior and abs(g1[1] - a_prior) <= SCALE_TOL * a_prior, (g1, a_prior)
        assert L[1] > -70 and abs(g1[-1] - a_prior) > 0.05 * a_prior          # measurable while SHORT, yet the prior is used
        s, L, g0, g1, flags, pcm, x, cuts = out[("silent-first", ramp)]
        assert flags[0] == SHORT | UNMEASURABLE and g1[0] == F32(32767.0) and g0[0] == g1[0], (flags, g1)
        assert g0[1] == F32(32767.0) and g1[1] != g0[1] and not flags[1] & UNMEASURABLE
        s, L, g0, g1, flags, pcm, x, cuts = out[("late-peak", ramp)]
        assert not flags[1] & LIMITED and flags[2] & LIMITED and all(f & LIMITED for f in flags[2:]) and g1[2] < g1[1], (flags, g1)
        assert g0[2] < g1[1] and g0[2] == g1[2] == F32(cap_of(ceiling_db, F32(0.9))), (g0, g1)      # g0 cut to the new cap
    return out


# ---- 4. what the feature is for ------------------------------------------------------------------------------------------
def delivered_loudness(pcm, fs):
    return Truth(np.asarray(pcm, np.float64) / 32767.0, fs).L


def click_rows(fs, seconds=2.0):
    """The same K-weighted content at very different peak-to-loudness ratios: a steady two-tone signal, and the same with a
    short click every 250 ms (3 samples wide, five times the tone's peak: under 1 LU of the loudness, 15 dB of the peak)."""
    n = int(seconds * fs)
    t = np.arange(n, dtype=np.float64) / fs
    base = 0.04 * np.sin(2 * np.pi * 330.0 * t) + 0.02 * np.sin(2 * np.pi * 1210.0 * t + 0.3)
    clicks = base.copy()
    for k in range(fs // 8, n - 3, fs // 4):
        clicks[k:k + 3] += np.array([0.28, -0.3, 0.25])
    return base.astype(F32), clicks.astype(F32)


def check_feature(eng, fs, T=-26.0, ceiling_db=-1.0, ramp=80):
    plain, clicks = click_rows(fs)
    h = (fs + 5) // 10
    cuts = [h + h // 2] * (plain.size // (h + h // 2))
    cuts.append(plain.size - sum(cuts))
    table = np.repeat(np.asarray(cuts, np.int32).reshape(-1, 1), 2, axis=1)
    _, _, _, _, pcm = eng.debug_stream_loudness([plain, clicks], fs, table, T, ceiling_db, None, ramp)
    mode3 = [delivered_loudness(p, fs) for p in pcm]
    # PE_GAIN_RUNNING on the same chunks, by its restatement (tests/emu/stream_gain_case.py): 32767 / running peak
    running = []
    for x in (plain, clicks):
        r, done, out = F32(0.01), 0, []
        for c in cuts:
            seg = x[done:done + c]
            r = max(r, F32(np.max(np.abs(seg))))
            out.append(np.clip(seg * (F32(32767.0) / r), F32(-32768.0), F32(32767.0)).astype(np.int16))
            done += c
        running.append(delivered_loudness(np.concatenate(out), fs))
    print(f"{fs} Hz, target {T}: delivered loudness plain / clicks: loudness mode {mode3[0]:.2f} / {mode3[1]:.2f} LUFS, "
          f"running mode {running[0]:.2f} / {running[1]:.2f} LUFS")
    for b in range(2):
        assert abs(mode3[b] - T) < abs(running[b] - T), (b, mode3, running)
    assert abs(mode3[0] - mode3[1]) < abs(running[0] - running[1]), (mode3, running)
    return mode3, running


# ---- 3. engine streams ------------------------------------------------------------------------------------------------
def drain_batch(eng, ids, nw, nz, chunk, scales):
    """Engine.stream_batch to its end in the loudness mode: per utterance the (float, int16, report) of every call."""
    B = len(ids)
    per = [[] for _ in ids]
    for item in eng.stream_batch(ids, scales, chunk_frames=chunk, noise_w=nw, noise_z=nz):
        L, g, p, f = eng.stream_last_loudness()
        g2, p2 = eng.stream_last_gains()
        assert L.shape == (B,) and np.array_equal(g, g2) and np.array_equal(p, p2)
        for b, (a, pc) in enumerate(item):
            per[b].append((a, pc, (L[b], g[b], p[b], f[b])))
    return per


def check_streams(per, fs, T, ceiling_db, prior, ramp, where):
    """Every call of every stream against the restatement on the engine's own floats; rows that have finished keep
    reporting their end state (Stream.chunk on an empty chunk). Returns the streams."""
    streams = []
    for b, calls in enumerate(per):
        s = Stream(fs, T, ceiling_db, prior, ramp)
        lastk = max(k for k, (a, _, _) in enumerate(calls) if a.size)
        for k, (a, pc, rep) in enumerate(calls):
            s.chunk(a, pc, rep, (where, b, k), last=k == lastk)
        streams.append(s)
    assert_exclusions(streams, str(where))
    return streams


def drain_one(eng, ids, scales, nw, nz, chunk):
    """Engine.stream (one utterance) to its end: [(float, int16, report)], and the report of the call that ended it."""
    calls = []
    for a, pc in eng.stream(ids, tuple(float(v) for v in scales), chunk_frames=chunk, noise_w=nw, noise_z=nz):
        L, g, p, f = eng.stream_last_loudness()
        g2, p2 = eng.stream_last_gains()
        assert L.shape == (1,) and g[0] == g2[0] and p[0] == p2[0]
        calls.append((a, pc, (L[0], g[0], p[0], f[0])))
    L, g, p, f = eng.stream_last_loudness()
    return calls, (L[0], g[0], p[0], f[0])


class Tenant:
    def __init__(self, x, stream):
        self.x, self.stream, self.n = x, stream, 0


def pool_scenario(eng, make_texts, join, slots, max_frames, chunk, T, ceiling_db, prior, ramp, between):
    """tests/emu/stream_gain_case.py's pool scenario for this mode. make_texts() -> fresh listeners [short, mid, long,
    fourth]; join(pool, listeners) -> slots; between(k): other calls on the handle between two chunks (0: a whole-utterance
    call, 1: one that grows the workspaces). Long and mid stream for two calls, short joins in mid-stream, a join without
    room fails and a refused setting changes nothing, short finishes and the fourth text takes the lowest free slot, long
    hangs up and short's text takes that slot. Every call's report of EVERY slot is held to the slot's own stream: a slot
    that delivers nothing keeps reporting its state, a reused slot starts from nothing."""
    from piper_amd.engine import EngineError
    fs = eng.output_rate
    t0, t1, t2, t3 = make_texts()
    eng.set_stream_loudness(T, ceiling_db, prior, ramp * 1000.0 / fs)
    assert eng.stream_gain[0] == "loudness" and eng.stream_loudness == (True, T, ceiling_db, prior, ramp)
    pool = eng.stream_pool(slots, max_frames)
    on, ended = {}, []
    empty_f, empty_i = np.zeros(0, F32), np.zeros(0, np.int16)

    def enter(xs):
        got = join(pool, xs)
        for x, s in zip(xs, got):
            if s in on:
                ended.append(on[s].stream)
            on[s] = Tenant(x, Stream(fs, T, ceiling_db, prior, ramp))
        return got

    def step():
        out = pool.next(chunk)
        L, g, p, f = eng.stream_last_loudness()
        assert L.shape == (pool.slots,)
        for s, t in on.items():
            a, pc = out.get(s, (empty_f, empty_i))
            t.stream.chunk(a, pc, (L[s], g[s], p[s], f[s]), ("pool", t.x.name, s, t.n))
            t.n += 1 if a.size else 0
        for s in range(pool.slots):
            if s not in on:
                assert tuple_eq((L[s], g[s], p[s], f[s]), EMPTY), s      # a slot nobody has taken yet
        return out

    assert enter([t2, t1]) == [0, 1]
    step()
    step()
    assert enter([t0]) == [2]
    between(0)
    step()
    between(1)
    nfree = len(pool.free_slots)
    try:
        join(pool, make_texts()[:nfree + 1])
        raise AssertionError("a join without room succeeded")
    except EngineError as e:
        assert "free slots" in str(e)
    setting = eng.stream_loudness
    for change in (lambda: eng.set_stream_loudness(-30.0, -2.0, None, 1.0), lambda: eng.set_stream_gain("fixed", 0.5)):
        try:
            change()
            raise AssertionError("the setting changed under an occupied pool")
        except EngineError as e:
            assert "occupied" in str(e) and eng.stream_loudness == setting
    step()
    newcomer = on[2]
    assert on[0].n == 4 and newcomer.n == 2
    while pool.frames_done[2] < t0.frames:
        step()
    free = pool.free_slots
    assert 2 in free and free[0] in on and on[free[0]].stream.r > 0          # the lowest free slot had a tenant
    was = on[free[0]].stream
    s3 = enter([t3])[0]
    assert s3 == free[0]
    step()
    # the new tenant's peak and loudness are its own first chunk's: nothing of the last tenant's stays
    assert on[s3].n == 1 and on[s3].stream.r == F32(np.max(np.abs(on[s3].stream.X))) and on[s3].stream.r != was.r
    assert pool.frames_done[0] < t2.frames and on[0].stream.r > 0
    pool.leave(0)
    assert enter([make_texts()[0]]) == [0]
    while step():
        pass
    assert on[0].n == newcomer.n
    # the same text alone in a slot that had a long tenant: the same loudness and gains as in the fresh slot it had before
    a, b = newcomer.stream.trace, on[0].stream.trace
    assert len(a) == len(b) and all(abs(u[2] - v[2]) <= 2 * L_TOL or u[2] == v[2] for u, v in zip(a, b)), (a, b)
    pool.close()
    streams = ended + [t.stream for t in on.values()]
    assert_exclusions(streams, "pool")
    eng.set_stream_gain("chunk")
    return streams
