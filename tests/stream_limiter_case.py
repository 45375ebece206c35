"""Look-ahead limiter on streams at a target loudness (pe_set_stream_limiter, kernels/stream_limiter.h): the f64 restatement of
DESIGN.md 4.9.1 and the cases shared by tests/test_stream_limiter_emu.py and tests/test_gpu_stream_limiter.py. The loudness
truth is tests/loudness_case.py's, the envelope's pieces (window, sliding minimum, conversion) tests/limiter_case.py's, the
stream's rule tests/stream_loudness_case.py's -- imported, not copied -- and no kernel is looked at.

With X the stream's floats, N_end its total, s_i the per-sample scale (step 7 of 4.9 from every chunk's {g0, g1, R}), C the
ceiling as an f32, W = max(1, floor(window_ms fs / 1000 + 0.5)), D = 2 W:

    g_i = (float)((double)s_i / 32767)
    r[i] = min(1, C / (g_i |X_i|)), 1 where X_i = 0 and outside [0, N_end)
    m, d, h, e as tests/limiter_case.py;  pcm_i = trunc(clamp((X_i e_i) s_i, +-floor(32767 C)))
    call k hands out the stream samples [b_(k-1), b_k): b_k = N_k where the call consumed the row's end, else max(0, N_k - D)

The bound of a device e against the f64 e formed from (X, s). g_i is part of the contract (one f32 rounding of an f64
quotient) and is taken as given, like g in limiter_case.py; from there on the stream's envelope IS limiter_case's with a
per-sample gain, and its derivation holds term by term: r 2 u, m and d 3 u, the sum u + 3 u + (2 W + 1) u, e u -- at most
bound(W) = (2 W + 6) u, u = 2^-24. That is the bound where s is known exactly: a chunk with g0 = g1 (fma(0, w, g1) = g1).
Inside a ramp the truth forms s_i = fma(g0 - g1, (R - 1 - i) / R, g1) from two roundings in f64 where the device has one
fma: the two may differ by one ulp of s, a relative 2^-23, which moves g_i |X_i| and with it r (<= 1) by at most 2^-23 = 2 u
where r < 1, and everything downstream is 1-Lipschitz in r. bound_ramped(W) = bound(W) + 2 u.

The int16 of a stream with varying gain against the untruncated f64 value v_i = clamp(X_i e_i s_i): the device forms
(X e) s in f32 with its own e and s -- |e_dev - e| <= bound, two f32 products (u each, relative) and the scale's ulp
(u relative, counted above in e only through r): |pcm_i - v_i| < 1 + (bound + 3 u) |X_i| s_i, the 1 for the truncation."""
import math

import numpy as np

import limiter_case as LM
import loudness_case as LC
import stream_loudness_case as S
from loudness_case import SHORT, LIMITED, SCALE_TOL, GATE_MARGIN

SHAPED = LM.SHAPED
F32 = np.float32
U = 2.0 ** -24
TILE = LM.TILE
CASES = ((8000, 5.0), (22050, 5.0), (48000, 5.0), (8000, 1.0), (8000, 10.0))


def window(fs, window_ms):
    W, _ = LM.window(fs, window_ms)
    return W, 2 * W


def bound(W):
    return LM.bound(W)


def bound_ramped(W):
    return LM.bound(W) + 2 * U


def delivered_counts(chunks, D):
    """The formula: per call the samples handed out, for one row cut into `chunks` (zeros allowed)."""
    last = max((k for k, c in enumerate(chunks) if c > 0), default=-1)
    N = b = 0
    out = []
    for k, c in enumerate(chunks):
        N += int(c)
        to = b if c == 0 else (N if k == last else max(0, N - D))
        out.append(to - b)
        b = to
    return out


def scales(chunks, g0, g1, R0):
    """s over the whole stream from every chunk's {g0, g1, R = min(R0, n)}, step 7 of 4.9: sample i < R of a chunk is scaled
    by fma(g0 - g1, (R - 1 - i) / R, g1) with the difference and the quotient in f32, every later one by g1. (The fma is
    formed in f64 and rounded: the one ulp that may cost is in bound_ramped.)"""
    out = []
    for c, a, b in zip(chunks, g0, g1):
        c = int(c)
        if c == 0:
            continue
        R = min(int(R0), c)
        s = np.full(c, F32(b), F32)
        if R > 0 and F32(a) != F32(b):
            w = (F32(R - 1) - np.arange(R, dtype=F32)) / F32(R)
            d = F32(a) - F32(b)
            s[:R] = (np.float64(d) * w.astype(np.float64) + np.float64(F32(b))).astype(F32)
        out.append(s)
    return np.concatenate(out) if out else np.zeros(0, F32)


def gains_of(s):
    return (s.astype(np.float64) / 32767.0).astype(F32)


def envelope(x, s, C, fs, window_ms):
    """(e, r) in f64 of a whole stream x with the per-sample scales s: limiter_case.envelope with a_i = g_i |X_i| standing
    for |x| at gain 1."""
    a = gains_of(s).astype(np.float64) * np.abs(np.asarray(x, np.float64))
    return LM.envelope(x, 1.0, C, fs, window_ms, a=a)


def value_f64(x, e, s, C):
    cq = math.floor(32767.0 * float(F32(C)))
    return np.clip(np.asarray(x, np.float64) * np.asarray(e, np.float64) * s.astype(np.float64), -cq, cq)


def check_pcm_bound(pcm, x, e, s, C, W, where):
    """Case 2's bound, and the ceiling on every sample."""
    v = value_f64(x, e, s, C)
    tol = 1.0 + (bound_ramped(W) + 3 * U) * np.abs(np.asarray(x, np.float64)) * s.astype(np.float64)
    err = np.abs(pcm.astype(np.float64) - v)
    assert np.all(err < tol), (where, int(np.argmax(err - tol)), float(np.max(err - tol)))
    assert int(np.max(np.abs(pcm.astype(np.int32)), initial=0)) <= math.floor(32767.0 * float(F32(C))), where


# ---- 1. composition at a constant gain ------------------------------------------------------------------------------------
T1, CEIL1 = -20.0, -1.0
PRIOR1 = float(F32(T1 - 20.0 * math.log10(2.0)))


def const_rows(fs, window_ms):
    """[(name, row)]: every row under 4 h samples, so that the stream stays SHORT and the prior sets the gain (a = 2)."""
    W, D = window(fs, window_ms)
    h = (fs + 5) // 10
    n = 12 * D + 37
    assert n < 4 * h
    rows = [("shaped", LM.TP.squashed(n, 7 * fs + W)), ("under", (0.3 * LM.TP.squashed(n, 7 * fs + W + 1)).astype(F32)),
            ("short", LM.TP.squashed(D - 1, 7 * fs + W + 2))]
    rows[2][1][(D - 1) // 2] = 0.97
    late = LM.quiet(n, fs + W + 3)
    late[n - 1 - W // 2] = 0.9
    early = LM.quiet(n, fs + W + 4)
    early[W // 2] = -0.9
    rows += [("peak-in-last-W", late), ("peak-in-first-W", early)]
    if fs == 8000 and window_ms == 5.0:
        rows.append(("tile-seam", LM.TP.squashed(4 * h - 1, 7 * fs + 5)))      # a LIM_TILE boundary inside the delivered range
        assert 4 * h - 1 > TILE
    return rows


def const_cuts(x, W, D):
    """Six ways to cut a row."""
    n = x.size

    def fill(c):
        c = max(1, c)
        return [c] * (n // c) + ([n % c] if n % c else [])

    def upto(points):
        out, done = [], 0
        for p in points:
            p = max(done, min(int(p), n))
            out.append(p - done)
            done = p
        out.append(n - done)
        return out

    p = int(np.argmax(np.abs(x)))
    mixed = upto(np.cumsum([W // 3, 0, 1, D, 0, 2 * D + 3, W]))
    return [[n], fill(W - 1), fill(D + 1), mixed,
            upto([p + D // 2 + 1, p + D // 2 + 1 + D + 3]),      # the peak in the last D samples of a chunk
            upto([max(0, p - D // 2), p + 2 * D])]               # ... and in the first D of one


def check_const(eng, fs, window_ms, R0):
    W, D = window(fs, window_ms)
    C = LM.ceiling_f32(CEIL1)
    rows = const_rows(fs, window_ms)
    xs = [x for _, x in rows]
    cuts = [const_cuts(x, W, D) for x in xs]
    ncut = len(cuts[0])
    got = [[] for _ in rows]
    worst = 0.0
    for call in range(ncut):
        pick = [cuts[b][(b + call) % ncut] for b in range(len(rows))]      # neighbouring rows are cut differently
        K = max(len(c) for c in pick)
        table = np.zeros((K, len(rows)), np.int32)
        for b, c in enumerate(pick):
            table[:len(c), b] = c
        L, g0, g1, flags, dl, env, pcm = eng.debug_stream_limiter(xs, fs, table, T1, CEIL1, PRIOR1, R0, window_ms)
        for b, (name, x) in enumerate(rows):
            where = (fs, window_ms, R0, name, call)
            assert list(dl[:, b]) == delivered_counts(table[:, b], D), (where, list(dl[:, b]))
            assert int(dl[:, b].sum()) == x.size
            live = table[:, b] > 0
            assert np.all(flags[live, b] & S.PRIOR) and np.all(flags[live, b] & SHORT), where
            assert np.all(g1[live, b] == g1[live, b][0]) and np.all(g0[live, b] == g1[live, b]), (where, g0[:, b], g1[:, b])
            got[b].append((env[b], pcm[b], F32(g1[live, b][0]), flags[live, b]))
    L3, _, g13, f3, pcm3 = eng.debug_stream_loudness(xs, fs, np.asarray([[x.size for x in xs]], np.int32), T1, CEIL1, PRIOR1, R0)
    for b, (name, x) in enumerate(rows):
        where = (fs, window_ms, R0, name)
        e0, p0, s0, _ = got[b][0]
        assert abs(float(s0) - 65534.0) <= SCALE_TOL * 65534.0, (where, s0)
        for e, p, s, _ in got[b][1:]:
            assert s == s0 and np.array_equal(e.view(np.int32), e0.view(np.int32)) and np.array_equal(p, p0), ("cuts differ", where)
        s = np.full(x.size, s0, F32)
        et, r = envelope(x, s, C, fs, window_ms)
        assert np.all(np.isfinite(e0)), where
        err = float(np.max(np.abs(e0.astype(np.float64) - et)))
        worst = max(worst, err / bound(W))
        assert err <= bound(W), (where, err, bound(W))
        assert np.array_equal(p0, LM.pcm_of(x, e0, s0, C)), where
        assert int(np.max(np.abs(p0.astype(np.int32)))) <= math.floor(32767.0 * float(C)), where
        over = np.flatnonzero(LM.envelope_f32_r(x, gains_of(s)[0], C) < 1.0)
        far = np.ones(x.size, bool)
        for i in over:
            far[max(0, i - 2 * W):i + 2 * W + 1] = False
        assert np.all(e0[far] == 1.0), where
        limited = [bool(np.any(f & LIMITED)) for _, _, _, f in got[b]]
        assert all(np.all((f & LIMITED != 0) == (f & SHAPED != 0)) for _, _, _, f in got[b]), where
        if name == "under":
            assert not over.size and not any(limited), where
        else:
            assert over.size and all(limited), where
        if not over.size:                                # never shaped: mode 3's int16, bit for bit
            assert g13[0, b] == s0 and not f3[0, b] & LIMITED, where
            assert np.array_equal(p0, pcm3[b]), where
    print(f"{fs} Hz, {window_ms} ms (W = {W}), ramp {R0}: {ncut} cuts agree bit for bit; worst envelope error "
          f"{worst:.3f} of the bound {bound(W):.2e}")
    return worst


# ---- 2. varying gain ----------------------------------------------------------------------------------------------------
T2, CEIL2 = -16.0, -3.0


def varying_rows(fs):
    """Rows of 8 to 13 segments without a prior: a tone that swells, a soft tone with a late click, noise bursts."""
    h = (fs + 5) // 10
    n = 9 * h + 13
    swell = (S.tone(n, fs, 0.03).astype(np.float64) * np.linspace(0.4, 2.5, n)).astype(F32)
    click_late = S.tone(8 * h, fs, 0.02)
    click_late[5 * h + 10] = 0.9
    burst = LC.bursts(13 * h + 7, fs, 11)
    return [("swell", swell), ("click-late", click_late), ("bursts", (0.2 * burst / max(1e-9, float(np.max(np.abs(burst))))).astype(F32))]


class Varying:
    """One row's stream through its chunks: the f64 rule on the prefix (S.rule with no running peak: the cap only marks),
    the gains held to it outside the gate margin, the flags, and s from what was reported."""

    def __init__(self, x, fs, ramp, y2):
        self.x, self.fs, self.ramp, self.y2 = x, fs, ramp, y2
        self.N, self.r, self.G, self.lu, self.first = 0, F32(0), None, None, True
        self.checked = self.excluded = 0
        self.chunks, self.g0, self.g1 = [], [], []
        self.limited = 0

    def chunk(self, c, L, g0, g1, flags, where, prior=None):
        c = int(c)
        if c == 0:
            return
        seg = self.x[self.N:self.N + c]
        self.N += c
        t = S.Prefix(self.x, self.y2, self.N, self.fs)
        r_new = max(self.r, F32(np.max(np.abs(seg))))
        t0, t1, tflags, lu = S.rule(t, T2, CEIL2, prior, 0.0, self.G, self.first, self.lu)
        cap = S.cap_of(CEIL2, r_new)
        self.checked += 1
        if t.margin < GATE_MARGIN:
            self.excluded += 1
        else:
            assert abs(float(g1) - t1) <= SCALE_TOL * t1, (where, self.N, float(g1), t1)
            assert int(flags) & ~(LIMITED | SHAPED) == tflags, (where, self.N, int(flags), tflags)
        # LIMITED | SHAPED exactly where the cap is under the device's own g1; g0 is the previous gain, uncut
        marked = (LIMITED | SHAPED) if cap < float(F32(g1)) else 0
        assert int(flags) & (LIMITED | SHAPED) == marked, (where, self.N, int(flags), cap, float(g1))
        self.limited += 1 if marked else 0
        assert F32(g0) == (F32(g1) if self.first else self.G_dev), (where, self.N, g0, g1)
        self.chunks.append(c)
        self.g0.append(F32(g0))
        self.g1.append(F32(g1))
        self.r, self.G, self.G_dev, self.lu, self.first = r_new, t1, F32(g1), lu, False


def check_varying(eng, fs, window_ms=5.0):
    W, D = window(fs, window_ms)
    C = LM.ceiling_f32(CEIL2)
    rows = varying_rows(fs)
    xs = [x for _, x in rows]
    y2 = [LC.kweight_sq(x, fs) for x in xs]
    cuts = [S.chunkings(x.size, fs) for x in xs]
    streams, worst, shaped_any = [], 0.0, False
    for ramp in (0, 64, 65536):
        for call in range(3):
            pick = [cuts[b][(b + call) % 3] for b in range(len(rows))]
            K = max(len(c) for c in pick)
            table = np.zeros((K, len(rows)), np.int32)
            for b, c in enumerate(pick):
                table[:len(c), b] = c
            L, g0, g1, flags, dl, env, pcm = eng.debug_stream_limiter(xs, fs, table, T2, CEIL2, None, ramp, window_ms)
            for b, (name, x) in enumerate(rows):
                where = (fs, name, ramp, call)
                assert list(dl[:, b]) == delivered_counts(table[:, b], D), where
                v = Varying(x, fs, ramp, y2[b])
                for k in range(K):
                    v.chunk(table[k, b], L[k, b], g0[k, b], g1[k, b], flags[k, b], where + (k,))
                streams.append(v)
                s = scales(v.chunks, v.g0, v.g1, ramp)
                assert s.size == x.size
                et, _ = envelope(x, s, C, fs, window_ms)
                err = float(np.max(np.abs(env[b].astype(np.float64) - et)))
                worst = max(worst, err / bound_ramped(W))
                assert np.all(np.isfinite(env[b])) and err <= bound_ramped(W), (where, err, bound_ramped(W))
                check_pcm_bound(pcm[b], x, et, s, C, W, where)
                shaped_any = shaped_any or bool(np.any(env[b] < 1.0))
                if name == "click-late":
                    assert v.limited and np.any(env[b] < 1.0), where
    S.assert_exclusions(streams, f"varying gain at {fs} Hz")
    assert shaped_any
    print(f"{fs} Hz, {window_ms} ms: worst envelope error {worst:.3f} of the bound {bound_ramped(W):.2e}")
    return worst


# ---- 3. what it is for --------------------------------------------------------------------------------------------------
def check_feature(eng, fs, T=-16.0, ceiling_db=-1.0, ramp=80, window_ms=5.0):
    """S.click_rows through mode 3 and through the limiter on the same chunks: the clicks row lands closer to the target,
    and the plain / clicks gap shrinks. Returns ((plain, clicks) in mode 3, (plain, clicks) with the limiter), LUFS."""
    plain, clicks = S.click_rows(fs)
    h = (fs + 5) // 10
    cuts = [h + h // 2] * (plain.size // (h + h // 2))
    cuts.append(plain.size - sum(cuts))
    table = np.repeat(np.asarray(cuts, np.int32).reshape(-1, 1), 2, axis=1)
    pcm3 = eng.debug_stream_loudness([plain, clicks], fs, table, T, ceiling_db, None, ramp)[4]
    out = eng.debug_stream_limiter([plain, clicks], fs, table, T, ceiling_db, None, ramp, window_ms)
    mode3 = [S.delivered_loudness(p, fs) for p in pcm3]
    limited = [S.delivered_loudness(p, fs) for p in out[6]]
    top = math.floor(32767.0 * float(LM.ceiling_f32(ceiling_db)))
    assert all(int(np.max(np.abs(p.astype(np.int32)))) <= top for p in out[6])
    print(f"{fs} Hz, target {T}: delivered loudness plain / clicks: mode 3 {mode3[0]:.2f} / {mode3[1]:.2f} LUFS, "
          f"with the limiter {limited[0]:.2f} / {limited[1]:.2f} LUFS")
    assert abs(limited[1] - T) < abs(mode3[1] - T), (mode3, limited)
    assert abs(limited[0] - limited[1]) < abs(mode3[0] - mode3[1]), (mode3, limited)
    return mode3, limited


# ---- 4. engine streams ----------------------------------------------------------------------------------------------------
class EngineStream:
    """One stream of the engine with the limiter on, call by call: the floats and int16 a call handed out, the report
    (L, g1, peak, flags) after it, and the chunk's own sample count n (known from the same stream in mode 3)."""

    def __init__(self, fs, ceiling_db, R0, window_ms):
        self.fs, self.cdb, self.R0, self.ms = fs, ceiling_db, int(R0), window_ms
        self.W, self.D = window(fs, window_ms)
        self.a, self.p, self.n, self.g0, self.g1, self.dl = [], [], [], [], [], []
        self.G = None
        self.limited = 0

    def call(self, a, pcm, report, n, where):
        assert a.dtype == np.float32 and pcm.dtype == np.int16 and a.size == pcm.size, where
        self.a.append(a)
        self.p.append(pcm)
        self.dl.append(a.size)
        self.n.append(int(n))
        if n:
            g1 = F32(report[1])
            self.g0.append(g1 if self.G is None else self.G)
            self.g1.append(g1)
            self.G = g1
            marked = int(report[3]) & (LIMITED | SHAPED)
            assert marked in (0, LIMITED | SHAPED), (where, int(report[3]))
            assert bool(marked) == (S.cap_of(self.cdb, F32(report[2])) < float(g1)), (where, report)
            self.limited += 1 if marked else 0

    def finish(self, base_floats, where):
        """base_floats: the stream's floats in mode 3. Returns (X, pcm, e of the truth)."""
        X = np.concatenate(self.a) if self.a else np.zeros(0, F32)
        P = np.concatenate(self.p) if self.p else np.zeros(0, np.int16)
        assert X.size == base_floats.size and np.array_equal(X.view(np.int32), base_floats.view(np.int32)), (where, X.size, base_floats.size)
        assert self.dl == delivered_counts(self.n, self.D), (where, self.dl, self.n, self.D)
        C = LM.ceiling_f32(self.cdb)
        s = scales([n for n in self.n if n], self.g0, self.g1, self.R0)
        e, _ = envelope(X, s, C, self.fs, self.ms)
        check_pcm_bound(P, X, e, s, C, self.W, where)
        return X, P, e, s


def mode3_pcm(X, s):
    """Mode 3's conversion of a stream with the scales s (clamp to the int16 range: nothing was LIMITED)."""
    return np.clip(np.asarray(X, F32) * s, F32(-32768.0), F32(32767.0)).astype(np.int16)


def check_report(stream, lims, e, s, X, where):
    """pe_stream_last_limiter of every call against the truth over the samples that call handed out. (X, s: the whole stream
    as far as it was generated -- what a listener who hung up never got still shaped what it did get.)"""
    C = float(LM.ceiling_f32(stream.cdb))
    W = stream.W
    bd = bound_ramped(W)
    a = gains_of(s).astype(np.float64) * np.abs(X.astype(np.float64))
    near = np.zeros(X.size, bool)
    for i in np.flatnonzero(a >= C * (1.0 - 4 * U)):
        near[max(0, i - 2 * W):i + 2 * W + 1] = True
    done = total = 0
    for k, (n, (red, cnt)) in enumerate(zip(stream.dl, lims)):
        ek = e[done:done + n]
        if n == 0:
            assert red == 0.0 and cnt == 0, (where, k, red, cnt)
            continue
        assert abs(float(red) - (1.0 - float(ek.min()))) <= bd, (where, k, float(red), 1.0 - float(ek.min()))
        assert int(np.sum(ek < 1.0 - bd)) <= int(cnt) <= int(np.sum(near[done:done + n])), (where, k, int(cnt))
        total += int(cnt)
        done += n
    return total


def run_stream(rec, base, fs, ceiling_db, R0, window_ms, where, left=False):
    """rec / base: per call (floats, int16, report, limiter report) of one stream with the limiter and of the same stream in
    mode 3 (whose chunks are the stream's own sample counts). left: the listener hung up -- what was held back is dropped.
    Returns the shaped samples reported."""
    assert len(rec) == len(base), (where, len(rec), len(base))
    st = EngineStream(fs, ceiling_db, R0, window_ms)
    for k, ((a, pc, rep, lim), (a0, _, _, _)) in enumerate(zip(rec, base)):
        st.call(a, pc, rep, a0.size, where + (k,))
    full = np.concatenate([a0 for a0, _, _, _ in base]) if base else np.zeros(0, F32)
    X = np.concatenate(st.a) if st.a else np.zeros(0, F32)
    P = np.concatenate(st.p) if st.p else np.zeros(0, np.int16)
    want = delivered_counts(st.n, st.D)
    if left:                                             # no call consumed the row's end
        last = max((k for k, c in enumerate(st.n) if c > 0), default=-1)
        if last >= 0:
            want[last] = max(0, sum(st.n) - st.D) - sum(want[:last])
    assert st.dl == want, (where, st.dl, want)
    assert np.array_equal(X.view(np.int32), full[:X.size].view(np.int32)), where
    assert left or X.size == full.size, where
    C = LM.ceiling_f32(ceiling_db)
    s = scales([n for n in st.n if n], st.g0, st.g1, R0)
    e, _ = envelope(full, s, C, fs, window_ms)
    shaped = check_report(st, [lim for _, _, _, lim in rec], e, s, full, where)
    e, s = e[:X.size], s[:X.size]
    check_pcm_bound(P, X, e, s, C, st.W, where)
    return shaped, st, (X, P, s)


def drain_batch(eng, ids, nw, nz, chunk, scales, limiter):
    """Engine.stream_batch to its end: per utterance and call (floats, int16, (L, g1, peak, flags), (max_reduction, shaped))."""
    B = len(ids)
    per = [[] for _ in ids]
    for item in eng.stream_batch(ids, scales, chunk_frames=chunk, noise_w=nw, noise_z=nz):
        L, g, p, f = eng.stream_last_loudness()
        red, cnt = eng.stream_last_limiter()
        assert L.shape == (B,) and red.shape == ((B,) if limiter else (0,))
        for b, (a, pc) in enumerate(item):
            per[b].append((a, pc, (L[b], g[b], p[b], f[b]), (red[b], cnt[b]) if limiter else (0.0, 0)))
    return per


def drain_one(eng, ids, scales, nw, nz, chunk, limiter):
    calls = []
    for a, pc in eng.stream(ids, tuple(float(v) for v in scales), chunk_frames=chunk, noise_w=nw, noise_z=nz):
        L, g, p, f = eng.stream_last_loudness()
        red, cnt = eng.stream_last_limiter()
        assert red.shape == ((1,) if limiter else (0,))
        calls.append((a, pc, (L[0], g[0], p[0], f[0]), (red[0], cnt[0]) if limiter else (0.0, 0)))
    return calls


def setting(eng, T, ceiling_db, R0, window_ms, limiter):
    fs = eng.output_rate
    eng.set_stream_loudness(T, ceiling_db, None, R0 * 1000.0 / fs, limiter=limiter, limiter_ms=window_ms)
    W, D = window(fs, window_ms)
    assert eng.stream_loudness == (True, T, ceiling_db, None, R0)
    assert eng.stream_limiter() == (limiter, window_ms, W, D) or not limiter and eng.stream_limiter()[0] is False


def check_batch(eng, inputs, chunk, scales, T, ceiling_db, R0, window_ms, where):
    """The ragged batch stream in mode 3 and with the limiter. Returns (shaped samples reported, streams, base)."""
    ids, nw, nz = inputs
    fs = eng.output_rate
    setting(eng, T, ceiling_db, R0, window_ms, False)
    base = drain_batch(eng, ids, nw, nz, chunk, scales, False)
    setting(eng, T, ceiling_db, R0, window_ms, True)
    per = drain_batch(eng, ids, nw, nz, chunk, scales, True)
    shaped, out = 0, []
    for b in range(len(ids)):
        n, st, xps = run_stream(per[b], base[b], fs, ceiling_db, R0, window_ms, where + (b,))
        shaped += n
        out.append((st, xps))
    eng.set_stream_gain("chunk")
    return shaped, out, base


def check_unlimited(out, base, where):
    """A target at which nothing is LIMITED: mode 3's int16 bit for bit, differing only in the call boundaries."""
    for b, ((st, (X, P, s)), calls) in enumerate(zip(out, base)):
        assert st.limited == 0, (where, b)
        assert not any(int(rep[3]) & LIMITED for _, _, rep, _ in calls), (where, b)
        assert np.array_equal(P, np.concatenate([pc for _, pc, _, _ in calls])), (where, b)
        assert st.D and any(d != n for d, n in zip(st.dl, st.n)), (where, b)      # (the boundaries did move)


def check_one(eng, inputs, b, chunk, scales, T, ceiling_db, R0, window_ms, where):
    ids, nw, nz = inputs
    fs = eng.output_rate
    setting(eng, T, ceiling_db, R0, window_ms, False)
    base = drain_one(eng, ids[b], scales[b], nw[b], nz[b], chunk, False)
    setting(eng, T, ceiling_db, R0, window_ms, True)
    rec = drain_one(eng, ids[b], scales[b], nw[b], nz[b], chunk, True)
    out = run_stream(rec, base, fs, ceiling_db, R0, window_ms, where + (b,))
    eng.set_stream_gain("chunk")
    return out[0], out[1:], base


def pool_run(eng, make_texts, join, chunk, limiter, between):
    """Three slots: long and mid stream for two calls; short joins in mid-stream with a first chunk of its own (2 frames);
    other calls on the handle between chunks; long hangs up in mid-stream and the fourth text, another speaker, takes its
    slot; then to the end. Returns {tenant name: (calls, left)} in joining order."""
    t0, t1, t2, t3 = make_texts()
    pool = eng.stream_pool(3, 48)
    on, log = {}, {}
    empty_f, empty_i = np.zeros(0, F32), np.zeros(0, np.int16)

    def enter(xs, tag):
        got = join(pool, xs)
        for x, s in zip(xs, got):
            on[s] = x.name + tag
            log[x.name + tag] = [[], False]
        return got

    def step(per_slot=None):
        out = pool.next(chunk, per_slot=per_slot)
        L, g, p, f = eng.stream_last_loudness()
        red, cnt = eng.stream_last_limiter()
        assert red.shape == ((pool.slots,) if limiter else (0,))
        live = set(int(s) for s in range(pool.slots) if s not in pool.free_slots) | set(out)
        for s, name in on.items():
            if log[name][1]:
                continue
            a, pc = out.get(s, (empty_f, empty_i))
            log[name][0].append((a, pc, (L[s], g[s], p[s], f[s]), (red[s], cnt[s]) if limiter else (0.0, 0)))
        return out, live

    assert enter([t2, t1], "") == [0, 1]
    step()
    step()
    assert enter([t0], "") == [2]
    between(0)
    step({2: 2})
    between(1)
    step()
    assert pool.frames_done[0] < t2.frames
    pool.leave(0)
    log[on[0]][1] = True
    assert enter([t3], "") == [0]
    for _ in range(64):
        step()
        if len(pool.free_slots) == pool.slots:
            break
    assert len(pool.free_slots) == pool.slots
    assert not pool.next(chunk)
    pool.close()
    return log


def check_pool(eng, make_texts, join, chunk, T, ceiling_db, R0, window_ms, between, where):
    fs = eng.output_rate
    setting(eng, T, ceiling_db, R0, window_ms, False)
    base = pool_run(eng, make_texts, join, chunk, False, between)
    setting(eng, T, ceiling_db, R0, window_ms, True)
    rec = pool_run(eng, make_texts, join, chunk, True, between)
    assert list(rec) == list(base)
    shaped, left_any = 0, False
    for name in rec:
        # (a finished tenant keeps its log growing with empty calls while its slot is not reused: cut to the base's length)
        n, st, _ = run_stream(rec[name][0], base[name][0], fs, ceiling_db, R0, window_ms, where + (name,), left=rec[name][1])
        shaped += n
        if rec[name][1]:
            left_any = True
            assert sum(st.dl) == max(0, sum(st.n) - st.D) and sum(st.n) > 0, (where, name)      # what was held back is gone
    assert left_any
    eng.set_stream_gain("chunk")
    return shaped


# ---- 5. refusals and idempotence --------------------------------------------------------------------------------------------
def check_refusals(make_engine, lib, K, P, make_onnx):
    """make_engine(preset) -> (cfg, engine); make_onnx() -> an engine of a voice without a header rate."""
    from piper_amd.engine import EngineError
    cfg, eng = make_engine()
    h, fs = eng._h, eng.output_rate
    ids, nw, nz = K.inputs(cfg)
    nan = float("nan")
    assert eng.stream_limiter() == (False, 5.0) + window(fs, 5.0)
    eng.set_stream_loudness(-18.0, -2.0, None, 3.0, limiter=True, limiter_ms=4.0)
    was, loud = eng.stream_limiter(), eng.stream_loudness
    assert was == (True, 4.0) + window(fs, 4.0) and was[3] == 2 * was[2] and loud[0] is True

    def fails(rc, text):
        assert rc != 0 and text in lib.pe_last_error().decode(), lib.pe_last_error()
        assert eng.stream_limiter() == was and eng.stream_loudness == loud

    for bad, text in ((0.5, "limiter window 0.5"), (10.5, "limiter window 10.5"), (-1.0, "limiter window -1"),
                      (nan, "limiter window nan"), (float("inf"), "limiter window inf")):
        fails(lib.pe_set_stream_limiter(h, 1, bad), text)
    # the Python surface sets both or neither
    for call in (lambda: eng.set_stream_loudness(-18.0, -2.0, None, 3.0, limiter=True, limiter_ms=11.0),
                 lambda: eng.set_stream_loudness(-3.0, -2.0, None, 3.0, limiter=False)):
        try:
            call()
            raise AssertionError("a bad value was accepted")
        except EngineError:
            assert eng.stream_limiter() == was and eng.stream_loudness == loud
    # not while a batch stream is live
    gen = eng.stream_batch(ids, K.SCALES, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)
    next(gen)
    fails(lib.pe_set_stream_limiter(h, 0, 0.0), "cannot change while a stream is live")
    fails(lib.pe_set_stream_limiter(h, 1, 5.0), "cannot change while a stream is live")
    for _ in gen:
        pass
    assert lib.pe_set_stream_limiter(h, 1, 6.0) == 0 and eng.stream_limiter()[:2] == (True, 6.0)
    # in the other modes it is remembered and nothing else changes
    eng.set_stream_gain("running", 0.05, 4.0)
    assert lib.pe_set_stream_limiter(h, 1, 7.0) == 0
    assert eng.stream_limiter()[:2] == (True, 7.0) and eng.stream_gain[0] == "running" and eng.stream_loudness[0] is False
    assert lib.pe_set_stream_limiter(h, 0, 0.0) == 0 and eng.stream_limiter()[:2] == (False, 7.0)
    eng.close()
    # not while a pool slot is occupied
    cfg, eng = make_engine("tiny-ms")
    h = eng._h
    eng.set_stream_loudness(-18.0, -2.0, None, 3.0, limiter=True, limiter_ms=4.0)
    was, loud = eng.stream_limiter(), eng.stream_loudness
    pool = eng.stream_pool(3, 48)
    P.join(pool, P.emu_texts(cfg, True)[:1])
    fails(lib.pe_set_stream_limiter(h, 0, 0.0), "stream pool slot is occupied")
    pool.next(K.CHUNK)
    fails(lib.pe_set_stream_limiter(h, 1, 2.0), "stream pool slot is occupied")
    pool.leave(0)
    assert lib.pe_set_stream_limiter(h, 1, 2.0) == 0 and eng.stream_limiter()[:2] == (True, 2.0)
    pool.close()
    eng.close()
    # a voice without a header rate has to be told its rate first
    onnx = make_onnx()
    assert lib.pe_set_stream_limiter(onnx._h, 1, 5.0) != 0 and "carries none" in lib.pe_last_error().decode()
    assert onnx.stream_limiter()[0] is False
    onnx.set_output_rate(None, native=16000)
    onnx.set_stream_loudness(-20.0, limiter=True)
    assert onnx.stream_limiter() == (True, 5.0, 80, 160)
    onnx.close()


def check_idempotence(eng, inputs, chunk, scales, T, ceiling_db, R0, window_ms):
    """Mode 3 before and after the limiter was on: the same int16, floats, reports, launches; no graph captured again."""
    ids, nw, nz = inputs

    def run(limiter):
        setting(eng, T, ceiling_db, R0, window_ms, limiter)
        eng.profile_enable(2)
        eng.profile_reset()
        per = drain_batch(eng, ids, nw, nz, chunk, scales, limiter)
        rows = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
        eng.profile_enable(0)
        return per, rows, eng.graph_stats[1]

    a, b, c, d = run(False), run(True), run(False), run(True)
    ncalls = len(a[0][0])
    assert "stream_limiter_kernel" not in a[1] and a[1].get("chunk_pcm_gain_kernel") == ncalls, a[1]
    assert b[1].get("stream_limiter_kernel") == ncalls and "chunk_pcm_gain_kernel" not in b[1], b[1]
    assert sum(b[1].values()) == sum(a[1].values()), (a[1], b[1])      # one launch in another's place
    assert a[1] == c[1] and b[1] == d[1]
    assert c[2] == b[2] and d[2] == b[2], (a[2], b[2], c[2], d[2])      # both sets of graphs stayed cached
    for x, y in ((a, c), (b, d)):
        for u, v in zip(x[0], y[0]):
            assert len(u) == len(v)
            for (a0, p0, r0, l0), (a1, p1, r1, l1) in zip(u, v):
                assert np.array_equal(a0, a1) and np.array_equal(p0, p1)
                assert S.tuple_eq(r0, r1) and float(l0[0]) == float(l1[0]) and int(l0[1]) == int(l1[1])
    eng.set_stream_gain("chunk")
