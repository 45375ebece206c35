"""Output-rate conversion (pe_set_output_rate): what tests/test_resample_emu.py and tests/test_gpu_resample.py share.

The filter is restated here in f64 numpy from its definition, not from the engine's table code. With fs_in the voice's rate
and fs_out the requested one:

    g = gcd(fs_in, fs_out), L = fs_out / g, M = fs_in / g, fmin = min(fs_in, fs_out), fc = 0.92 * fmin / 2
    Z = 16, beta = 8.6, Th = Z / (2 fc)
    h(t) = (2 fc / fs_in) sinc(2 fc t) I0(beta sqrt(1 - (t / Th)^2)) / I0(beta)      for |t| <= Th, else 0
    y[n] = sum_j x[j] h(n / fs_out - j / fs_in),   x[j] = 0 outside the utterance

The argument of h is exactly (n M - j L) / (L M g): it is formed from the integer numerator. An utterance of S native
samples has ceil(S L / M) outputs; the taps of output n lie within K = ceil(Z fs_in / (0.92 fmin)) native samples of
floor(n M / L).

The a-priori bound of every pointwise comparison: an f32 dot product of T terms whose coefficients were rounded once from
f64, summed in any order, with or without FMA, is within (T + 3) 2^-24 sum_j |h| |x[j]| of the exact sum (T = the taps of
that output inside the window's support; T + 1 roundings by the standard forward analysis, the rest is room for a
coefficient whose f64 value sits on a rounding boundary and for the second-order terms). Derived, not measured."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

Z, BETA = 16.0, 8.6


def params(fs_in, fs_out):
    g = math.gcd(fs_in, fs_out)
    fmin = min(fs_in, fs_out)
    fc = 0.92 * fmin / 2.0
    return SimpleNamespace(fs_in=fs_in, fs_out=fs_out, g=g, L=fs_out // g, M=fs_in // g, fmin=fmin, fc=fc,
                           Th=Z / (2.0 * fc), K=int(math.ceil(Z * fs_in / (0.92 * fmin))))


def n_out(S, fs_in, fs_out):
    p = params(fs_in, fs_out)
    return -((-int(S) * p.L) // p.M)


def h(t, p):
    u = t / p.Th
    inside = np.abs(u) <= 1.0
    w = np.i0(BETA * np.sqrt(np.clip(1.0 - u * u, 0.0, None))) / np.i0(BETA)
    return np.where(inside, (2.0 * p.fc / p.fs_in) * np.sinc(2.0 * p.fc * t) * w, 0.0), inside


def truth(x, fs_in, fs_out, n0=0, count=None, origin=0):
    """Outputs n0 .. n0 + count - 1 of the utterance whose native samples origin .. origin + len(x) - 1 are x (zero
    elsewhere), in f64, and the bound of the module docstring for each. count None: every output of an utterance that IS x."""
    p = params(fs_in, fs_out)
    x = np.asarray(x, np.float64)
    if count is None:
        assert n0 == 0 and origin == 0
        count = n_out(x.size, fs_in, fs_out)
    y, bound = np.zeros(count), np.zeros(count)
    d = np.arange(-p.K - 1, p.K + 2, dtype=np.int64)
    den = float(p.L) * float(p.M) * float(p.g)
    for a in range(0, count, 8192):
        n = n0 + np.arange(a, min(count, a + 8192), dtype=np.int64)
        j = (n * p.M // p.L)[:, None] + d[None, :]
        hh, inside = h((n[:, None] * p.M - j * p.L).astype(np.float64) / den, p)
        i = j - origin
        ok = (i >= 0) & (i < x.size)
        xv = np.where(ok, x[np.clip(i, 0, max(x.size - 1, 0))] if x.size else 0.0, 0.0)
        y[a:a + n.size] = (hh * xv).sum(axis=1)
        bound[a:a + n.size] = (inside.sum(axis=1) + 3) * 2.0 ** -24 * (np.abs(hh) * np.abs(xv)).sum(axis=1)
    return y, bound


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the samples (0 / 0 counts as 0: an output no tap reaches must be exactly zero)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max()) if r.size else 0.0


def assert_within(got, want, bound, what):
    assert np.asarray(got).shape == want.shape, (what, np.asarray(got).shape, want.shape)
    r = worst_ratio(got, want, bound)
    print(f"{what}: {want.size} samples, worst |error| / bound = {r:.3f}")
    assert r <= 1.0, (what, r)
    return r


def tone_figures(y, f, fs_out, skip):
    """Least-squares fit of a tone of frequency f to y without `skip` samples at each end: (gain in dB of the fitted
    amplitude over 1, rms of what the fit leaves over the fitted tone's rms in dB)."""
    n = np.arange(y.size, dtype=np.float64)[skip:y.size - skip]
    v = np.asarray(y, np.float64)[skip:y.size - skip]
    A = np.stack([np.cos(2 * np.pi * f * n / fs_out), np.sin(2 * np.pi * f * n / fs_out)], axis=1)
    c, *_ = np.linalg.lstsq(A, v, rcond=None)
    fit = A @ c
    amp = float(np.hypot(c[0], c[1]))
    res = float(np.sqrt(np.mean((v - fit) ** 2)))
    return 20 * np.log10(amp), 20 * np.log10(max(res, 1e-300) / (amp / np.sqrt(2.0)))


def level_db(y, skip):
    """rms of y without `skip` samples at each end over the rms of a unit tone, in dB."""
    v = np.asarray(y, np.float64)[skip:y.size - skip]
    return 20 * np.log10(max(float(np.sqrt(np.mean(v * v))), 1e-300) * np.sqrt(2.0))


def chunk_count(f0, f1, hop, fs_in, fs_out):
    return n_out(f1 * hop, fs_in, fs_out) - n_out(f0 * hop, fs_in, fs_out)


def check_chunks(chunks, sizes, native, hop, fs_in, fs_out, O, what, cut=False):
    """chunks: [(float, int16)] delivered at fs_out for chunk sizes `sizes` (frames); native: the float chunks of the same
    utterance at its own rate. Counts per chunk, the concatenation against the f64 resampling of the concatenated native
    chunks, every chunk's int16 against the conversion rule on its floats. cut: the utterance went on after the last
    chunk (the listener left), so the outputs whose taps reach past the last delivered native sample -- K native samples,
    ceil(K L / M) + 1 outputs at the most -- have no truth here and are left out."""
    f = 0
    for k, ((a, p), c) in enumerate(zip(chunks, sizes)):
        assert a.size == p.size == chunk_count(f, f + c, hop, fs_in, fs_out), (what, k, a.size, f, c)
        assert p.dtype == np.int16 and np.array_equal(O.audio_float_to_int16(a), p), (what, k)
        f += c
    x = np.concatenate(native)
    assert x.size == f * hop, (what, x.size, f, hop)
    want, bound = truth(x, fs_in, fs_out, n0=0, count=n_out(f * hop, fs_in, fs_out))
    got = np.concatenate([a for a, _ in chunks])
    if cut:
        q = params(fs_in, fs_out)
        keep = want.size - (-(-q.K * q.L // q.M) + 1)
        got, want, bound = got[:keep], want[:keep], bound[:keep]
    return assert_within(got, want, bound, what)


def play_pool(eng, texts, chunk, first, slots=None, max_frames=48):
    """The scenario of tests/stream_pool_case.py (its module docstring: text 2 alone for two calls, texts 0 and 1 join with
    a first chunk of `first` frames, text 3 takes the finished text 0's slot, the resident with the most frames to come
    leaves, drain), at whatever rate the engine delivers: sample counts are not assumed to be frames x hop. Fills every
    listener's chunks / sizes; returns the halo the pool reported."""
    import stream_pool_case as P
    t0, t2, t3 = texts[0], texts[2], texts[3]
    second = [texts[0], texts[1]]
    slots = slots or 3
    pool = eng.stream_pool(slots, max_frames)
    try:
        assert P.join(pool, [t2]) == [0]
        on, pending = {0: t2}, {}
        calls = since_t3 = 0
        someone_left = False
        while True:
            calls += 1
            assert calls < 200
            before = pool.frames_done
            out = pool.next(chunk, per_slot=pending or None)
            done = pool.frames_done
            if not out:
                break
            for s in range(slots):
                x, got = on.get(s), int(done[s] - before[s])
                if x is None or x.left or got == 0:
                    assert s not in out and got == 0, (calls, s)
                    continue
                assert got == min(pending.get(s, chunk), x.frames - int(before[s])), (calls, s)
                x.chunks.append(out[s])
                x.sizes.append(got)
            pending = {}
            if calls == 2:
                assert P.join(pool, second) == [1, 2]
                for x in second:
                    on[x.slot] = x
                    pending[x.slot] = first
            if t3.slot is not None:
                since_t3 += 1
                if since_t3 == 2:
                    live = [x for x in on.values() if not x.left and done[x.slot] < x.frames]
                    assert live
                    x = max(live, key=lambda x: (x is not t3, x.frames - int(done[x.slot])))
                    pool.leave(x.slot)
                    x.left = someone_left = True
            elif t0.slot is not None and done[t0.slot] == t0.frames:
                free = pool.free_slots
                assert t0.slot in free
                assert P.join(pool, [t3]) == [free[0]]
                on[t3.slot] = t3
                pending = {t3.slot: first}
        assert t3.slot is not None and someone_left
        return pool.halo
    finally:
        pool.close()
