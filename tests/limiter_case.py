"""Look-ahead limiter of the target loudness (pe_set_loudness_limiter, kernels/limiter.h): the f64 restatement of the contract
in include/piper_hip.h and the cases shared by tests/test_limiter_emu.py and tests/test_gpu_limiter.py. The loudness truth is
tests/loudness_case.py's, the true-peak truth tests/true_peak_case.py's (imported, not copied).

With x[0 .. n) a row at rate fs, g the gain of its loudness target, C the ceiling:

    W = max(1, floor(window_ms fs / 1000 + 0.5))
    r[i] = min(1, C / (g |x[i]|)), 1 where x[i] = 0 and outside [0, n)
    m[j] = min r[j - W .. j + W],  d = 1 - m
    e[i] = min(r[i], 1 - sum_{k = -W .. W} h_k d[i + k]),  h_k = H_k / sum H,  H_k = (1 + cos(pi k / (W + 1))) / 2
    pcm[i] = trunc(clamp((x[i] e[i]) scale, +-floor(32767 C))),  scale = 32767 g

The bound of a device e against the f64 e (bound(W) below), with g and C the device's own f32 values as inputs. Errors are
absolute, u = 2^-24 (every quantity lies in [0, 1], where one f32 rounding is at most u / 2; u is used for each):
    r       g |x| and the quotient round once each, the min is exact: 2 u (r <= 1)
    m, d    min is 1-Lipschitz, 1 - m rounds once: 3 u
    sum     the weights are rounded once from f64: sum |dh_k| d <= u; the errors of d enter with weights that sum to 1: 3 u;
            every fma of the 2 W + 1 taps rounds a partial sum below 1: (2 W + 1) u
    e       1 - sum rounds once: u; the outer min is 1-Lipschitz in both arguments
which is at most (2 W + 6) u, second-order terms aside.

With the true-peak ceiling a[i] = max(|x[i]|, v[i - 1], v[i]) stands for |x[i]|, v[c] = max over ph of |y[c Q + ph]|, y the
interpolation of tests/true_peak_case.py (v[-1] = 0). The device's v lies within dv of the f64 one, dv the largest per-output
bound resample_case.truth returns for the row (max is 1-Lipschitz). r = C / (g a) has |dr / da| = C / (g a^2) < g / C wherever
r < 1 (a > C / g), and where one side is clamped to 1 the difference is smaller still: r moves by at most dv g / C, and so
does everything downstream (min and the weighted sum are 1-Lipschitz in r). bound_true = bound(W) + 1.01 dv g / C."""
import math

import numpy as np

import loudness_case as LC
import true_peak_case as TP          # noqa: F401  (the true-peak truth, for callers of this module)

SHAPED = 8
TILE = 2048             # samples one workgroup of limiter_kernel covers (kernels/params.h: LIM_TILE)
RATES = (8000, 16000, 48000)
WINDOWS = (1.0, 5.0, 10.0)
CEILING = -1.0
GAIN = 2.0              # gain of the kernel rows: squashed noise (peaks near 1) is shaped, 0.3 x noise is not


def window(fs, window_ms):
    """(W, h[2 W + 1]) of the definition, f64."""
    W = max(1, int(math.floor(window_ms * fs / 1000.0 + 0.5)))
    k = np.arange(-W, W + 1, dtype=np.float64)
    H = 0.5 * (1.0 + np.cos(np.pi * k / (W + 1)))
    return W, H / H.sum()


def bound(W):
    return (2 * W + 6) * 2.0 ** -24


def peaks_v(x, fs):
    """(v, dv): v[c] = max over the Q phases of |y[c Q + ph]| in f64, and the bound of a device v against it."""
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return np.zeros(0), 0.0
    Q = TP.oversample(fs)
    y, b = TP.R.truth(x, fs, Q * fs)
    assert y.size == x.size * Q
    return np.abs(y).reshape(x.size, Q).max(axis=1), float(b.max())


def a_true(x, fs):
    """(a, dv) of the true-peak ceiling: max(|x[i]|, v[i - 1], v[i])."""
    v, dv = peaks_v(x, fs)
    a = np.abs(np.asarray(x, np.float64))
    if a.size:
        a = np.maximum(a, v)
        a[1:] = np.maximum(a[1:], v[:-1])
    return a, dv


def bound_true(W, g, C, dv):
    return bound(W) + 1.01 * dv * float(g) / float(C)


def trim_truth(z, fs, g, C):
    """(trim, P, bound of the device's t_z) of shaped floats z: min(1, C / (g max(p_z, t_z)))."""
    pz = float(np.max(np.abs(z))) if len(z) else 0.0
    tz, tb, _ = TP.true_peak(np.asarray(z, np.float32), fs)
    P = max(pz, tz)
    return (min(1.0, float(C) / (float(g) * P)) if P > 0 else 1.0), P, tb


def ceiling_f32(ceiling_db):
    """C as the engine holds it: 10^(dB / 20) computed in f64 and rounded once."""
    return np.float32(10.0 ** (float(ceiling_db) / 20.0))


def scale_of(g):
    """The conversion's scale of a gain: one f32 product."""
    return np.float32(32767.0) * np.float32(g)


def device_gain(scale):
    """The g limiter_kernel works with: its f32 scale / 32767 in f64, rounded once."""
    return np.float32(np.float64(np.float32(scale)) / 32767.0)


def shaped(x, g, ceiling_db):
    """The rule of loudness_gain_kernel: the ceiling's term is the smaller one (C / P < g)."""
    p = float(np.max(np.abs(x))) if len(x) else 0.0
    return p > 0.0 and float(ceiling_f32(ceiling_db)) / p < float(np.float32(g))


def sliding_min(r, W):
    """m[j] = min r[j - W .. j + W] for j in [-W, n + W), r = 1 outside [0, n)."""
    n = r.size
    rp = np.concatenate([np.ones(2 * W), r, np.ones(2 * W)])
    m = np.ones(n + 2 * W)
    for k in range(2 * W + 1):
        m = np.minimum(m, rp[k:k + n + 2 * W])
    return m


def envelope(x, g, C, fs, window_ms, a=None):
    """(e, r) in f64 of one row; g and C are taken as given (the device's own f32 values). a: |x| or what stands for it."""
    W, h = window(fs, window_ms)
    a = np.abs(np.asarray(x, np.float64)) if a is None else np.asarray(a, np.float64)
    r = np.ones(a.size)
    nz = a > 0
    r[nz] = np.minimum(1.0, float(C) / (float(g) * a[nz]))
    if a.size == 0:
        return r, r
    d = 1.0 - sliding_min(r, W)                          # d[j], j in [-W, n + W)
    s = np.convolve(d, h[::-1], mode="valid")            # sum_k h_k d[i + k], i in [0, n)
    assert s.size == a.size
    return np.minimum(r, 1.0 - s), r


def envelope_f32_r(x, g, C):
    """r as the kernel forms it, every operation in f32."""
    a = np.abs(np.asarray(x, np.float32))
    r = np.ones(a.size, np.float32)
    nz = a > 0
    with np.errstate(over="ignore", divide="ignore"):
        r[nz] = np.minimum(np.float32(1.0), np.float32(C) / (np.float32(g) * a[nz]))
    return r


def pcm_of(x, e, scale, C):
    """The f32 restatement of the conversion: trunc(clamp((x e) scale, +-floor(32767 C)))."""
    cq = np.float32(math.floor(32767.0 * float(np.float32(C))))
    v = (np.asarray(x, np.float32) * np.asarray(e, np.float32)) * np.float32(scale)
    return np.clip(v, -cq, cq).astype(np.int16)


def pcm_f64(x, e, scale, C):
    """The f64 conversion, before truncation."""
    cq = math.floor(32767.0 * float(np.float32(C)))
    return np.clip(np.asarray(x, np.float64) * np.asarray(e, np.float64) * float(scale), -cq, cq)


# ---- the kernel cases -------------------------------------------------------------------------------------------------
def quiet(n, seed, amp=0.1):
    return (amp * np.tanh(3.0 * np.random.default_rng(seed).standard_normal(n))).astype(np.float32)


def kernel_rows(fs, window_ms):
    """[(name, row)] of the ragged batch of one rate and window. With GAIN = 2 and C = -1 dB: squashed noise (peaks near 1)
    is shaped at almost every sample; the quiet rows (amplitude 0.1) lie under the ceiling but for the samples set to 0.9."""
    W, _ = window(fs, window_ms)
    T = TILE
    rows = []
    for k, n in enumerate((0, 1, 2, W, 2 * W, 2 * W + 1, 4 * W + 1, T - 1, T, T + 1, 2 * T + 3)):
        x = TP.squashed(n, 100 * fs + k)
        if n:
            x[n // 2] = 0.97                             # (shaped whatever the noise drew)
        rows.append((f"noise[{n}]#{k}", x))
    n = T + 4 * W + 7
    for name, at in (("first", [0]), ("last", [n - 1]), ("seam-1", [T - 1]), ("seam", [T]),
                     ("apart2W", [300, 300 + 2 * W]), ("apart2W+1", [300, 300 + 2 * W + 1])):
        x = quiet(n, fs + len(rows))
        for i in at:
            x[i] = 0.9 if i % 2 else -0.9
        rows.append((name, x))
    x = quiet(n, fs + 77)
    x[200:200 + 6 * W + 9] = 0.8
    rows.append(("plateau", x))
    rows.append(("under", quiet(T + 100, fs + 78, amp=0.3)))
    rows.append(("zeros", np.zeros(T + 100, np.float32)))
    return rows


def check_kernel_true(eng, fs, window_ms):
    """check_kernel with the true-peak ceiling: the envelope within bound_true of the f64 one formed from a = max(|x|, v[i-1],
    v[i]); e <= r and e == 1 away from every peak, with the margins of dv; the int16 against the conversion of z = x e_dev
    with the f64 scale 32767 min(g, C / max(p_z, t_z)), under 32767 C, and its f64 true peak under C + S / 32767. Returns
    (worst error as a fraction of the bound, smallest trim)."""
    rows = kernel_rows(fs, window_ms)
    W, _ = window(fs, window_ms)
    C, S = ceiling_f32(CEILING), TP.truncation_slack(fs)
    g = np.full(len(rows), GAIN, np.float32)
    xs = [x for _, x in rows]
    e1, p1 = eng.debug_limiter(xs, fs, g, CEILING, 1, window_ms, pad=np.nan)
    e2, p2 = eng.debug_limiter(xs, fs, g, CEILING, 1, window_ms, pad=np.nan)
    worst, least = 0.0, 1.0
    for b, (name, x) in enumerate(rows):
        tag = (fs, window_ms, name, "TRUE")
        assert np.array_equal(e1[b].view(np.int32), e2[b].view(np.int32)) and np.array_equal(p1[b], p2[b]), ("two runs differ", tag)
        scale = scale_of(g[b])
        a, dv = a_true(x, fs)
        amax = float(a.max()) if a.size else 0.0
        is_shaped = amax > 0 and float(C) / amax < float(g[b])
        assert abs(float(g[b]) * amax / float(C) - 1.0) > 1e-3 or not amax, tag       # (no row sits on the rule's edge)
        if not is_shaped:
            assert name in ("under", "zeros") or x.size == 0, tag
            assert np.all(e1[b] == 1.0) and np.array_equal(p1[b], LC.pcm_of(x, scale)), tag
            continue
        gd = device_gain(scale)
        bt = bound_true(W, gd, C, dv)
        e, r = envelope(x, gd, C, fs, window_ms, a=a)
        err = float(np.max(np.abs(e1[b].astype(np.float64) - e)))
        worst = max(worst, err / bt)
        assert np.all(np.isfinite(e1[b])) and err <= bt, (tag, err, bt)
        assert np.all(e1[b].astype(np.float64) <= r + bt), tag
        over = np.flatnonzero(float(gd) * a >= float(C) * (1.0 - dv * float(gd) / float(C) - 4 * 2.0 ** -24))
        assert over.size, tag
        far = np.ones(x.size, bool)
        for i in over:
            far[max(0, i - 2 * W):i + 2 * W + 1] = False
        assert np.all(e1[b][far] == 1.0), tag
        z = x * e1[b]                                     # f32, as the kernel forms it
        trim, P, tb = trim_truth(z, fs, gd, C)
        least = min(least, trim)
        s = float(scale) * trim
        cq = math.floor(32767.0 * float(C))
        want = np.clip(z.astype(np.float64) * s, -cq, cq)
        tol = 1.0 + np.ceil(np.abs(z.astype(np.float64)) * s * (tb / P + 2.0 ** -22))
        assert np.all(np.abs(p1[b].astype(np.float64) - want) <= tol), (tag, float(np.max(np.abs(p1[b] - want))))
        assert int(np.max(np.abs(p1[b].astype(np.int32)))) <= 32767.0 * float(C), tag
        delivered = TP.true_peak(p1[b].astype(np.float64) / 32767.0, fs)[0]
        assert delivered <= float(C) + S / 32767.0, (tag, delivered)
    print(f"{fs} Hz, {window_ms} ms (W = {W}), TRUE: worst envelope error {worst:.3f} of the bound, smallest trim "
          f"{20 * math.log10(least):.4f} dB")
    return worst, least


def check_kernel(eng, fs, window_ms):
    """debug_limiter on the rows as one ragged batch whose padding behind every row's end is NaN, twice: the envelope within
    bound(W) of the f64 truth formed with the device's own g and C, the runs bit-equal, and the exact properties. Returns
    the worst error as a fraction of the bound."""
    rows = kernel_rows(fs, window_ms)
    W, _ = window(fs, window_ms)
    C = ceiling_f32(CEILING)
    g = np.full(len(rows), GAIN, np.float32)
    xs = [x for _, x in rows]
    e1, p1 = eng.debug_limiter(xs, fs, g, CEILING, 0, window_ms, pad=np.nan)
    e2, p2 = eng.debug_limiter(xs, fs, g, CEILING, 0, window_ms, pad=np.nan)
    worst = 0.0
    for b, (name, x) in enumerate(rows):
        tag = (fs, window_ms, name)
        assert e1[b].size == x.size == p1[b].size
        assert np.array_equal(e1[b].view(np.int32), e2[b].view(np.int32)) and np.array_equal(p1[b], p2[b]), ("two runs differ", tag)
        scale = scale_of(g[b])
        if not shaped(x, g[b], CEILING):
            assert name in ("under", "zeros") or x.size == 0, tag
            assert np.all(e1[b] == 1.0), tag
            assert np.array_equal(p1[b], LC.pcm_of(x, scale)), tag      # pcm16_gain_kernel's conversion
            continue
        gd = device_gain(scale)
        e, r = envelope(x, gd, C, fs, window_ms)
        err = float(np.max(np.abs(e1[b].astype(np.float64) - e))) if x.size else 0.0
        worst = max(worst, err / bound(W))
        assert np.all(np.isfinite(e1[b])), tag
        assert err <= bound(W), (tag, err, bound(W))
        r32 = envelope_f32_r(x, gd, C)
        assert np.all(e1[b] <= r32), tag
        over = np.flatnonzero(r32 < 1.0)
        assert over.size, tag
        far = np.ones(x.size, bool)
        for i in over:
            far[max(0, i - 2 * W):i + 2 * W + 1] = False
        assert np.all(e1[b][far] == 1.0), tag
        assert np.array_equal(p1[b], pcm_of(x, e1[b], scale, C)), tag
        assert int(np.max(np.abs(p1[b].astype(np.int32)))) <= 32767.0 * float(C), tag
        if name in ("seam-1", "seam"):
            # continuous across the tile seam: the step between the two samples is the truth's, within the bound
            i = TILE
            assert abs((float(e1[b][i]) - float(e1[b][i - 1])) - (e[i] - e[i - 1])) <= 2 * bound(W), tag
            assert e1[b][i] < 1.0 and e1[b][i - 1] < 1.0, tag
        if name == "plateau":
            inside = slice(200 + 2 * W, 200 + 4 * W + 9)
            assert np.max(np.abs(e1[b][inside].astype(np.float64) - r[inside])) <= bound(W), tag
            assert np.ptp(r[inside]) == 0.0
        if name == "apart2W":                            # the windows touch: no sample between the peaks is released
            assert np.all(e1[b][300:300 + 2 * W + 1] < 1.0), tag
    print(f"{fs} Hz, {window_ms} ms (W = {W}): worst envelope error {worst:.3f} of the bound {bound(W):.2e}")
    return worst


# ---- whole utterances -------------------------------------------------------------------------------------------------
def delivered_loudness(pcm, fs):
    return LC.Truth(np.asarray(pcm, np.float64) / 32767.0, fs)


def check_delivery(eng, r, off, fs, target, ceiling_db, window_ms, label="", kind=0):
    """A Synthesis `r` of a call with the loudness and the limiter on (sample-peak ceiling) and `off`, the same call with the
    limiter off: equal floats; flags against the f64 rule; for a shaped row the report and the int16 against the f64
    envelope formed with the device's g (reported scale / 32767), |pcm| <= 32767 C, and a delivered loudness strictly
    nearer the target than the limiter-off delivery; every other row bit-equal to the limiter-off row. kind = 1, the
    true-peak ceiling: the rule with P = max(p, t), the envelope from a = max(|x|, v[i - 1], v[i]) within bound_true, the
    trim against the f64 one, and the f64 true peak of the delivered int16 under C + S / 32767. Returns the flags."""
    L, scale, peak, flags = eng.last_loudness()
    red, cnt, trim = eng.last_limiter()
    assert L.size == len(r.audio) == red.size == cnt.size == trim.size == len(off.audio)
    W, _ = window(fs, window_ms)
    C = ceiling_f32(ceiling_db)
    for b, (a, pcm) in enumerate(zip(r.audio, r.pcm)):
        tag = f"{label}utterance {b} ({a.size} samples at {fs} Hz)"
        assert a.size and np.array_equal(a.view(np.int32), off.audio[b].view(np.int32)), tag
        lt = LC.Truth(a, fs)
        assert lt.margin >= LC.GATE_MARGIN, (tag, lt.margin)
        if kind:
            want_scale, want_flags = TP.scale_true(lt, TP.true_peak(a, fs)[0], target, ceiling_db)
        else:
            want_scale, want_flags = lt.scale(target, ceiling_db)
        is_shaped = bool(want_flags & LC.LIMITED) and not want_flags & LC.UNMEASURABLE
        assert int(flags[b]) == want_flags | (SHAPED if is_shaped else 0), (tag, int(flags[b]), want_flags)
        if not kind:
            assert np.float32(trim[b]) == np.float32(1.0), tag
        if not is_shaped:
            assert red[b] == 0.0 and cnt[b] == 0 and trim[b] == 1.0, tag
            assert np.array_equal(pcm, off.pcm[b]), tag
            continue
        g1 = 10.0 ** ((target - lt.L) / 20.0)
        # (the reported scale is the one that was used: the target's gain times the trim)
        assert abs(float(scale[b]) / float(trim[b]) - 32767.0 * g1) <= LC.SCALE_TOL * 32767.0 * g1, (tag, float(scale[b]), 32767.0 * g1)
        gd = device_gain(np.float32(float(scale[b]) / float(trim[b])))
        if kind:
            av, dv = a_true(a, fs)
            e, _ = envelope(a, gd, C, fs, window_ms, a=av)
            bd = bound_true(W, gd, C, dv) + (4 * 2.0 ** -24 if trim[b] < 1.0 else 0.0)
            tt, P, tb = trim_truth(a.astype(np.float64) * e, fs, gd, C)
            print(f"{tag}: trim {float(trim[b]):.7f} (f64 {tt:.7f})")
            assert abs(float(trim[b]) - tt) <= (bd * float(np.max(np.abs(a))) + tb) / P + 1e-6, (tag, float(trim[b]), tt)
            delivered = TP.true_peak(pcm.astype(np.float64) / 32767.0, fs)[0]
            assert delivered <= float(C) + TP.truncation_slack(fs) / 32767.0, (tag, delivered)
        else:
            e, _ = envelope(a, gd, C, fs, window_ms)
            bd = bound(W)
        # the count of e < 1 against the f64 one: a sample whose f64 e lies within the bound of 1 may read 1 on the device,
        # and a sample whose g |x| lies within 4 u of C may count as over the ceiling on one side only (+- 2 W around it)
        lo, hi = int(np.sum(e < 1.0 - bd)), int(np.sum(e < 1.0))
        edge = np.flatnonzero(np.abs(float(gd) * (av if kind else np.abs(a.astype(np.float64))) / float(C) - 1.0)
                              <= 4 * 2.0 ** -24 + (dv * float(gd) / float(C) if kind else 0.0))
        hi += edge.size * (4 * W + 1)
        print(f"{tag}: scale {float(scale[b]):.3f}, max reduction {float(red[b]):.6f} (f64 {1.0 - float(e.min()):.6f}), shaped samples "
              f"{int(cnt[b])} (f64 {hi}), flags {int(flags[b])}")
        assert abs(float(red[b]) - (1.0 - float(e.min()))) <= bd, (tag, float(red[b]), 1.0 - float(e.min()))
        assert lo <= int(cnt[b]) <= hi, (tag, int(cnt[b]), lo, hi)
        want = pcm_f64(a, e, np.float32(scale[b]), C)
        tol = 1.0 + np.ceil(float(scale[b]) * np.abs(a.astype(np.float64)) * bd)
        assert np.all(np.abs(pcm.astype(np.float64) - want) <= tol), (tag, float(np.max(np.abs(pcm - want))))
        assert int(np.max(np.abs(pcm.astype(np.int32)))) <= 32767.0 * float(C), tag
        on_l, off_l = delivered_loudness(pcm, fs), delivered_loudness(off.pcm[b], fs)
        print(f"{tag}: delivered {on_l.L:.3f} LUFS with the limiter, {off_l.L:.3f} without (target {target})")
        assert on_l.margin >= LC.GATE_MARGIN and off_l.margin >= LC.GATE_MARGIN, (tag, on_l.margin, off_l.margin)
        assert abs(on_l.L - target) < abs(off_l.L - target), (tag, on_l.L, off_l.L, target)
    return flags


# ---- the clicks row ---------------------------------------------------------------------------------------------------
def clicks(fs, seconds=3.0, seed=5):
    """Noise at 0.1 amplitude with four clicks of 0.9: the row of the issue, one plosive-like peak per 0.6 s."""
    n = int(seconds * fs)
    x = (0.1 * np.random.default_rng(seed + fs).uniform(-1.0, 1.0, n)).astype(np.float32)
    for k in range(4):
        x[int((0.4 + 0.6 * k) * fs)] = 0.9 if k % 2 else -0.9
    return x


def check_clicks(eng, fs, target, window_ms=5.0):
    """The clicks row through debug_limiter with g = 10^((T - L) / 20), L the f64 loudness, against the limiter-off rule:
    (shortfall with the limiter, shortfall without), in dB, of the f64 loudness of the delivered int16."""
    x = clicks(fs)
    lt = LC.Truth(x, fs)
    assert lt.margin >= LC.GATE_MARGIN, lt.margin
    g = np.float32(10.0 ** ((target - lt.L) / 20.0))
    assert shaped(x, g, CEILING)
    _, pcm = eng.debug_limiter([x], fs, [g], CEILING, 0, window_ms)
    off_scale, off_flags = lt.scale(target, CEILING)
    assert off_flags & LC.LIMITED
    on_l, off_l = delivered_loudness(pcm[0], fs), delivered_loudness(LC.pcm_of(x, np.float32(off_scale)), fs)
    assert on_l.margin >= LC.GATE_MARGIN and off_l.margin >= LC.GATE_MARGIN, (on_l.margin, off_l.margin)
    assert int(np.max(np.abs(pcm[0].astype(np.int32)))) <= 32767.0 * float(ceiling_f32(CEILING))
    print(f"clicks at {fs} Hz, T {target}: shortfall {target - on_l.L:.3f} dB with the limiter, {target - off_l.L:.3f} dB without")
    return target - on_l.L, target - off_l.L
