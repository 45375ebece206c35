"""Target loudness (pe_set_loudness, kernels/loudness.h): the f64 restatement of the contract in include/piper_hip.h and the
cases shared by tests/test_loudness_emu.py and tests/test_gpu_loudness.py. Nothing here looks at the kernels: the filter is
the plain serial direct form in Python floats (f64), the blocks and gates are the sums of ITU-R BS.1770-4 written out."""
import math

import numpy as np

SHORT, UNMEASURABLE, LIMITED = 1, 2, 4
L_TOL = 1e-3            # LU: 20 x the error of a plain f32 serial direct form on these signals, 100 x below audibility
SCALE_TOL = 2e-4        # relative (1e-3 LU is 1.15e-4 in gain)
GATE_MARGIN = 0.01      # LU: no block of a test signal lies this close to a gate, so rounding cannot flip one

# ITU-R BS.1770-4, table 1 and 2 (48000 Hz)
TABLE_48K = dict(shelf_b=(1.53512485958697, -2.69169618940638, 1.19839281085285),
                 shelf_a=(-1.69065929318241, 0.73248077421585),
                 hp_a=(-1.99004745483398, 0.99007225036621))


def coefficients(fs):
    """[shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2] by the bilinear transform of the analog prototypes."""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return shelf + hp


class Truth:
    """L, flags and everything the gates saw, of one row."""

    def __init__(self, x, fs):
        x = np.asarray(x, np.float32)
        n, h = x.size, (fs + 5) // 10
        self.n, self.h, self.peak = n, h, float(np.max(np.abs(x))) if n else 0.0
        self.flags, self.L, self.margin = 0, -math.inf, math.inf
        self.dropped_abs = self.dropped_rel = 0
        if n == 0:
            self.flags = SHORT | UNMEASURABLE
            return
        y2 = kweight_sq(x, fs)
        if n < 4 * h:
            self.flags = SHORT
            z = float(np.sum(y2)) / n
            l = -0.691 + 10.0 * math.log10(z) if z > 0 else -math.inf
            self.margin = abs(l + 70.0)
            if l > -70.0:
                self.L = l
            else:
                self.flags |= UNMEASURABLE
            return
        nseg = n // h
        s = [float(np.sum(y2[j * h:(j + 1) * h])) for j in range(nseg)]
        z = np.asarray([(s[j] + s[j + 1] + s[j + 2] + s[j + 3]) / (4.0 * h) for j in range(nseg - 3)], np.float64)
        with np.errstate(divide="ignore"):
            l = -0.691 + 10.0 * np.log10(z)
        self.blocks = l
        keep = l > -70.0
        self.dropped_abs = int(np.sum(~keep))
        self.margin = float(np.min(np.abs(l + 70.0)))
        if not keep.any():
            self.flags = UNMEASURABLE
            return
        gamma = -0.691 + 10.0 * math.log10(float(np.mean(z[keep]))) - 10.0
        self.gamma = gamma
        self.margin = min(self.margin, float(np.min(np.abs(l - gamma))))
        keep2 = keep & (l > gamma)
        self.dropped_rel = int(np.sum(keep & ~keep2))
        self.L = -0.691 + 10.0 * math.log10(float(np.mean(z[keep2])))

    def scale(self, target, ceiling_db):
        """(scale, flags) of the f64 formula."""
        if self.flags & UNMEASURABLE or not self.peak > 0:
            return 32767.0, self.flags | UNMEASURABLE
        g1, g2 = 10.0 ** ((target - self.L) / 20.0), 10.0 ** (ceiling_db / 20.0) / self.peak
        return 32767.0 * min(g1, g2), self.flags | (LIMITED if g2 < g1 else 0)


def kweight_sq(x, fs):
    """y^2 of the K-weighted row (f64)."""
    b0, b1, b2, a1, a2, c0, c1, c2, d1, d2 = coefficients(fs)
    xs = np.asarray(x, np.float64).tolist()
    out = [0.0] * len(xs)
    x1 = x2 = y1 = y2 = u1 = u2 = 0.0
    for i, v in enumerate(xs):
        y = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        u = c0 * y + c1 * y1 + c2 * y2 - d1 * u1 - d2 * u2
        x2, x1, y2, y1, u2, u1 = x1, v, y1, y, u1, u
        out[i] = u * u
    return np.asarray(out, np.float64)


def pcm_of(audio, scale):
    """pcm16_kernel's conversion with a given f32 scale: multiply in f32, clamp, truncate."""
    v = np.asarray(audio, np.float32) * np.float32(scale)
    return np.clip(v, np.float32(-32768.0), np.float32(32767.0)).astype(np.int16)      # (astype truncates toward zero)


# ---- the kernel cases -------------------------------------------------------------------------------------------------
RATES = (8000, 16000, 22050, 48000)


def lengths(fs):
    h = (fs + 5) // 10
    return [0, 1, h - 1, 4 * h - 1, 4 * h, 4 * h + 1, 5 * h - 1, 5 * h, 13 * h + 7]


def bursts(n, fs, seed):
    """A loud burst (400 ms), a pause of noise at -80 dBFS (500 ms: two whole blocks fall to the absolute gate), a soft burst
    40 dB under the loud one (to the end: its whole blocks fall to the relative gate); tones plus noise, cut to n samples."""
    h = (fs + 5) // 10
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    tone = 0.6 * np.sin(2 * np.pi * 310.0 * t) + 0.3 * np.sin(2 * np.pi * 1370.0 * t + 0.4) + 0.1 * rng.standard_normal(n)
    env = np.full(n, 0.3 * 10.0 ** (-40.0 / 20.0))
    env[:4 * h] = 0.3
    env[4 * h:9 * h] = 0.0
    x = env * tone
    pause = slice(min(n, 4 * h), min(n, 9 * h))
    x[pause] = 1e-4 * rng.standard_normal(x[pause].size)
    return x.astype(np.float32)


def kernel_rows(fs):
    """[(name, row)]: the bursts at every length of lengths(fs), a row with a DC offset, an all-zero row, and -- at 48000 Hz
    -- the standard's calibration tone, a full-scale 997 Hz sine of one second."""
    h = (fs + 5) // 10
    rows = [(f"bursts[{n}]", bursts(n, fs, fs + k)) for k, n in enumerate(lengths(fs))]
    t = np.arange(5 * h + 3, dtype=np.float64) / fs
    rows.append(("dc", (0.2 + 0.25 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)))
    rows.append(("zeros", np.zeros(6 * h, np.float32)))
    if fs == 48000:
        rows.append(("sine997", np.sin(2 * np.pi * 997.0 * np.arange(fs, dtype=np.float64) / fs).astype(np.float32)))
    return rows


def check_rows(eng, fs, rows, target=-23.0, ceiling_db=-1.0, label=""):
    """debug_loudness on the rows as one ragged batch, twice: every row against its f64 truth, the runs bit-equal. Returns
    {name: (truth, L)}."""
    got = eng.debug_loudness([r for _, r in rows], fs, target, ceiling_db)
    again = eng.debug_loudness([r for _, r in rows], fs, target, ceiling_db)
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "two runs differ"
    L, scale, flags = got
    out = {}
    for b, (name, x) in enumerate(rows):
        t = Truth(x, fs)
        want_scale, want_flags = t.scale(target, ceiling_db)
        tag = f"{label}{fs} Hz, {name}"
        print(f"{tag}: L {float(L[b]):.6f} (f64 {t.L:.6f}), scale {float(scale[b]):.4f} (f64 {want_scale:.4f}), flags "
              f"{int(flags[b])}, gate margin {t.margin:.3f} LU")
        assert t.margin >= GATE_MARGIN, (tag, t.margin)
        assert int(flags[b]) == want_flags, (tag, int(flags[b]), want_flags)
        if want_flags & UNMEASURABLE:
            assert L[b] == -np.inf and scale[b] == np.float32(32767.0), (tag, L[b], scale[b])
        else:
            assert abs(float(L[b]) - t.L) <= L_TOL, (tag, float(L[b]), t.L)
            assert abs(float(scale[b]) - want_scale) <= SCALE_TOL * want_scale, (tag, float(scale[b]), want_scale)
        out[name] = (t, float(L[b]))
    return out


def check_kernel(eng, fs):
    h = (fs + 5) // 10
    res = check_rows(eng, fs, kernel_rows(fs))
    long_t = res[f"bursts[{13 * h + 7}]"][0]
    assert long_t.dropped_abs >= 1 and long_t.dropped_rel >= 1, (long_t.dropped_abs, long_t.dropped_rel)
    assert res["zeros"][0].flags & UNMEASURABLE and not res["dc"][0].flags
    for n in lengths(fs):
        assert bool(res[f"bursts[{n}]"][0].flags & SHORT) == (n < 4 * h), n
    if fs == 48000:
        t, L = res["sine997"]
        assert abs(t.L + 3.0103) < 1e-3 and abs(L + 3.01) <= 0.01, (t.L, L)


# ---- whole utterances -------------------------------------------------------------------------------------------------
def check_delivery(eng, r, fs, target, ceiling_db, label=""):
    """A Synthesis of a call with the setting on: the report against the f64 loudness of the engine's own delivered floats,
    and the int16 as the conversion of those floats with the reported scale."""
    L, scale, peak, flags = eng.last_loudness()
    assert L.size == len(r.audio)
    for b, (a, p) in enumerate(zip(r.audio, r.pcm)):
        t = Truth(a, fs)
        want_scale, want_flags = t.scale(target, ceiling_db)
        tag = f"{label}utterance {b} ({a.size} samples at {fs} Hz)"
        print(f"{tag}: L {float(L[b]):.5f} (f64 {t.L:.5f}), scale {float(scale[b]):.3f} (f64 {want_scale:.3f}), flags {int(flags[b])}, "
              f"gate margin {t.margin:.3f} LU")
        assert t.margin >= GATE_MARGIN, (tag, t.margin)
        assert np.float32(peak[b]) == np.float32(t.peak), (tag, peak[b], t.peak)
        assert int(flags[b]) == want_flags, (tag, int(flags[b]), want_flags)
        if not want_flags & UNMEASURABLE:
            assert abs(float(L[b]) - t.L) <= L_TOL, (tag, float(L[b]), t.L)
        assert abs(float(scale[b]) - want_scale) <= SCALE_TOL * want_scale, (tag, float(scale[b]), want_scale)
        assert np.array_equal(pcm_of(a, scale[b]), p), tag
        if want_flags & LIMITED:
            assert int(np.max(np.abs(p.astype(np.int32)))) <= 32767.0 * 10.0 ** (ceiling_db / 20.0), tag
    return L, scale, peak, flags
