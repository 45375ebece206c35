"""True-peak ceiling of the target loudness (pe_set_loudness_ceiling, kernels/true_peak.h): the f64 restatement of the
contract in include/piper_hip.h and the cases shared by tests/test_true_peak_emu.py and tests/test_gpu_true_peak.py.

With x[0 .. n) the floats a whole-utterance call delivers at the rate fs:

    Q = ceil(192000 / fs)
    y = x interpolated Q times by the project's filter for the pair fs -> Q fs (tests/resample_case.py: truth, imported,
        not copied), y[m] for m = 0 .. n Q - 1, x = 0 outside [0, n)
    t = max |y[m]| (0 for n == 0),  P = max(p, t),  p = max |x|
    scale = 32767 min(10^((T - L) / 20), C / P), LIMITED when the second term is the smaller

The bound of every comparison of a device t with the f64 one is the largest per-output bound resample_case.truth returns
for the row: every output is within its own bound there (derived in that module), and max is 1-Lipschitz."""
import math

import numpy as np

import loudness_case as LC
import resample_case as R

K = 18                  # half-width of the interpolator in samples of x, at every rate
TILE = 1024             # T: native samples one workgroup of true_peak_kernel covers (kernels/params.h: TP_TILE)
RATES = (8000, 16000, 22050, 48000)
SAMPLE, TRUE = 0, 1
TONE_AMP = 0.5
TONE_SKIP = 200


def oversample(fs):
    return -(-192000 // fs)


def true_peak(x, fs):
    """(t, bound, argmax in units of samples of x) of one row, in f64."""
    x = np.asarray(x, np.float32)
    if x.size == 0:
        return 0.0, 0.0, 0.0
    Q = oversample(fs)
    y, bound = R.truth(x, fs, Q * fs)
    assert y.size == x.size * Q
    m = int(np.argmax(np.abs(y)))
    return float(np.abs(y[m])), float(bound.max()), m / Q


def filter_f64(fs):
    """[Q][2 K] table of the definition: row ph holds the taps of outputs c Q + ph on x[c - K + 1 .. c + K]."""
    Q = oversample(fs)
    p = R.params(fs, Q * fs)
    assert (p.L, p.M, p.K) == (Q, 1, K)
    ph, k = np.arange(Q)[:, None], np.arange(2 * K)[None, :]
    h, _ = R.h((ph + (K - 1 - k) * Q).astype(np.float64) / (float(p.L) * float(p.M) * float(p.g)), p)
    return h


def truncation_slack(fs):
    """S: the largest per-phase sum |h|. Truncating every sample of a row by less than one int16 step moves any interpolated
    value by less than S steps."""
    return float(np.abs(filter_f64(fs)).sum(axis=1).max())


def squashed(n, seed):
    return np.tanh(3.0 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


_STRADDLE = {}


def straddle_row(fs):
    """A squashed-noise row of TILE + 64 samples, quiet (x 0.3) but for the six samples around index TILE, whose largest
    inter-sample excursion lies within one sample of TILE, the boundary between the kernel's tiles 0 and 1: the first seed
    for which the f64 argmax does (searched on the CPU, asserted by the caller)."""
    if fs not in _STRADDLE:
        for seed in range(64):
            x = squashed(TILE + 64, 7000 + seed)
            env = np.full(x.size, 0.3, np.float32)
            env[TILE - 3:TILE + 3] = 1.0
            x = x * env
            t, _, at = true_peak(x, fs)
            p = float(np.max(np.abs(x)))
            if abs(at - TILE) <= 1.0 and at != round(at) and t > 1.05 * p:
                _STRADDLE[fs] = x
                break
        else:
            raise AssertionError(f"no straddling row found at {fs} Hz")
    return _STRADDLE[fs]


def kernel_rows(fs):
    """[(name, row)] of the ragged batch of one rate."""
    T = TILE
    rows = [(f"noise[{n}]", squashed(n, fs + k)) for k, n in enumerate((0, 1, 2, K - 1, K, 2 * K + 1, T - 1, T, T + 1, 2 * T + 3))]
    n = np.arange(2000, dtype=np.float64)
    rows.append(("quarter", (TONE_AMP * np.sin(2 * np.pi * n / 4.0 + np.pi / 4.0)).astype(np.float32)))
    # the same tone faded in and out over TONE_SKIP samples: the one number the device returns for it is a reading away
    # from the row's ends, where the abrupt onset of "quarter" overshoots
    fade = np.ones(2000)
    fade[:TONE_SKIP] = 0.5 - 0.5 * np.cos(np.pi * np.arange(TONE_SKIP) / TONE_SKIP)
    fade[-TONE_SKIP:] = fade[:TONE_SKIP][::-1]
    rows.append(("quarter_faded", (TONE_AMP * fade * np.sin(2 * np.pi * n / 4.0 + np.pi / 4.0)).astype(np.float32)))
    rows.append(("tone997", (0.8 * np.sin(2 * np.pi * 997.0 * np.arange(1500, dtype=np.float64) / fs)).astype(np.float32)))
    first, last = np.zeros(300, np.float32), np.zeros(T + 5, np.float32)
    first[0], last[-1] = 1.0, 1.0
    rows += [("impulse_first", first), ("impulse_last", last)]
    rows.append(("dc", np.full(700, 0.25, np.float32)))
    rows.append(("zeros", np.zeros(T + 100, np.float32)))
    rows.append(("straddle", straddle_row(fs)))
    return rows


_TRUTH = {}


def kernel_truth(fs):
    """{name: (t, bound, argmax)} of kernel_rows(fs), computed once."""
    if fs not in _TRUTH:
        _TRUTH[fs] = {name: true_peak(x, fs) for name, x in kernel_rows(fs)}
    return _TRUTH[fs]


def check_kernel(eng, fs):
    """debug_true_peak on the rows as one ragged batch whose padding behind every row's end is NaN, twice: every row within
    its bound of the f64 truth, the runs bit-equal, and the properties of the single rows."""
    rows, truth = kernel_rows(fs), kernel_truth(fs)
    Q = oversample(fs)
    got = eng.debug_true_peak([x for _, x in rows], fs, pad=np.nan)
    again = eng.debug_true_peak([x for _, x in rows], fs, pad=np.nan)
    assert np.array_equal(got.view(np.int32), again.view(np.int32)), "two runs differ"
    res = {}
    for b, (name, x) in enumerate(rows):
        t, bound, at = truth[name]
        p = float(np.max(np.abs(x))) if x.size else 0.0
        print(f"{fs} Hz, {name}: t {float(got[b]):.7f} (f64 {t:.7f}, bound {bound:.2e}, error {abs(float(got[b]) - t):.2e}), "
              f"p {p:.7f}, argmax at {at:.3f}")
        assert np.isfinite(got[b]), (fs, name)
        assert abs(float(got[b]) - t) <= bound, (fs, name, float(got[b]), t, bound)
        res[name] = (float(got[b]), p)
    assert abs(truth["straddle"][2] - TILE) <= 1.0, truth["straddle"]
    assert res["zeros"][0] == 0.0 and res["noise[0]"][0] == 0.0
    for name in ("impulse_first", "impulse_last"):
        t, p = res[name]
        assert p == 1.0 and 0.9 < t < p, (name, t, p)
    # the fs / 4 tone sampled at 45 degrees: its samples read -3.01 dB, its true peak 0 dB of the tone's amplitude, within
    # the filter's 0.07 dB and the distance of the nearest phase from the crest (half a step of 1 / Q sample at odd Q). The
    # reading is taken away from the row's ends, whose abrupt onset overshoots (0.12 dB, which the device reads too and is
    # held to above): in f64 over the row without TONE_SKIP samples at either end, and on the device from the faded row
    x = rows[[n for n, _ in rows].index("quarter")][1]
    y, _ = R.truth(x, fs, Q * fs)
    inner = float(np.max(np.abs(y[TONE_SKIP * Q:y.size - TONE_SKIP * Q])))
    tol = 0.07 + abs(20 * math.log10(math.cos(math.pi / (4 * Q))))
    t, p = res["quarter"]
    print(f"{fs} Hz, quarter: sample peak {20 * math.log10(p / TONE_AMP):.3f} dB, true peak {20 * math.log10(t / TONE_AMP):.3f} dB "
          f"(f64 away from the ends {20 * math.log10(inner / TONE_AMP):.3f} dB), tolerance {tol:.3f} dB")
    assert abs(20 * math.log10(p / TONE_AMP) + 3.0103) <= 0.001
    assert abs(20 * math.log10(inner / TONE_AMP)) <= tol
    faded = res["quarter_faded"][0]
    print(f"{fs} Hz, quarter_faded: true peak {20 * math.log10(faded / TONE_AMP):.3f} dB")
    assert abs(20 * math.log10(faded / TONE_AMP)) <= tol and abs(20 * math.log10(res["quarter_faded"][1] / TONE_AMP) + 3.0103) <= 0.001
    return res, inner


# ---- whole utterances -------------------------------------------------------------------------------------------------
def scale_true(truth, t, target, ceiling_db):
    """(scale, flags) of the f64 formula with P = max(p, t); truth: loudness_case.Truth of the row."""
    P = max(truth.peak, t)
    if truth.flags & LC.UNMEASURABLE or not P > 0:
        return 32767.0, truth.flags | LC.UNMEASURABLE
    g1, g2 = 10.0 ** ((target - truth.L) / 20.0), 10.0 ** (ceiling_db / 20.0) / P
    return 32767.0 * min(g1, g2), truth.flags | (LC.LIMITED if g2 < g1 else 0)


def check_delivery(eng, r, fs, target, ceiling_db, label=""):
    """A Synthesis of a call with the loudness on and the kind TRUE: the reported true peak against the f64 one of the
    delivered floats, scale and flags against the f64 formula with P, the int16 the conversion with the reported scale, and
    the f64 true peak of what is delivered under the ceiling (+ S int16 steps of truncation) wherever the ceiling won.
    Returns [(flags, f64 true peak of pcm / 32767)]."""
    L, scale, peak, flags = eng.last_loudness()
    tp = eng.last_true_peak()
    assert L.size == len(r.audio) == tp.size
    C, S = 10.0 ** (ceiling_db / 20.0), truncation_slack(fs)
    out = []
    for b, (a, pcm) in enumerate(zip(r.audio, r.pcm)):
        lt = LC.Truth(a, fs)
        t, bound, _ = true_peak(a, fs)
        want_scale, want_flags = scale_true(lt, t, target, ceiling_db)
        tag = f"{label}utterance {b} ({a.size} samples at {fs} Hz)"
        delivered, _, _ = true_peak(pcm.astype(np.float64) / 32767.0, fs)
        print(f"{tag}: t {float(tp[b]):.6f} (f64 {t:.6f}, bound {bound:.1e}), p {float(peak[b]):.6f}, scale {float(scale[b]):.3f} "
              f"(f64 {want_scale:.3f}), flags {int(flags[b])}, delivered true peak {delivered:.5f} (ceiling {C:.5f})")
        assert lt.margin >= LC.GATE_MARGIN, (tag, lt.margin)
        assert abs(float(tp[b]) - t) <= bound, (tag, float(tp[b]), t, bound)
        assert np.float32(peak[b]) == np.float32(lt.peak), (tag, peak[b], lt.peak)
        assert int(flags[b]) == want_flags, (tag, int(flags[b]), want_flags)
        assert abs(float(scale[b]) - want_scale) <= LC.SCALE_TOL * want_scale, (tag, float(scale[b]), want_scale)
        assert np.array_equal(LC.pcm_of(a, scale[b]), pcm), tag
        if want_flags & LC.LIMITED or not want_flags & LC.UNMEASURABLE:
            assert delivered <= C + S / 32767.0, (tag, delivered, C, S)
        out.append((int(flags[b]), delivered))
    return out
