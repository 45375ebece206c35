"""Speaker blends and caller-supplied speaker vectors (include/piper_hip.h: pe_blend): what
tests/test_speaker_blend_emu.py (the kernel emulator) and tests/test_gpu_speaker_blend.py (an MI355X) share. numpy and the
oracle only, no device of its own.

The law. Utterance b of a call gets one speaker vector g_b[gin]: the table row of its plain id; for components
(s_0, a_0) .. (s_{n-1}, a_{n-1}), n <= 8, per element g = a_0 * e_{s_0}[i] as one f32 product, then
g = fmaf(a_k, e_{s_k}[i], g) in the order given; or the caller's own vector, bit for bit. Everything behind g_b is the plain
call's arithmetic, so the truth for ANY g is the oracle run on the one-row table g[None] with sid = 0.

Bounds. The vector against the law in f64: |g - g64| <= 8 * 2^-24 * sum_k |a_k e_k| per element -- n <= 8 roundings of half
an ulp of a partial sum that never exceeds the absolute sum. Exact for a plain id and for a vector. Two runs fed identical
noise and the same g are held to seeds_case.PCM_LSB against each other, like the seeded-independence tests."""
import numpy as np

from oracle import vits_oracle as O
from piper_amd import weights as W

SCALES = (0.6, 1.0, 0.7)
LENS = (9, 4, 12)
SPEAKERS = [{1: 0.7, 3: 0.3}, {2: 1.0}, {0: 1.5, 1: -0.5}]
NOISE_SEED = 21
W_MARGIN = 1e-3          # every oracle w in front of the ceil stays this far from an integer (0.0090 with the inputs above)
BLEND_MAX = 8


def table(w):
    return np.ascontiguousarray(w["emb_g.weight"], np.float32)


def ids_of(cfg, lens=LENS):
    return [W.synthetic_phoneme_ids(T, i, id_max=cfg.n_vocab - 1) for i, T in enumerate(lens)]


def noise(cfg, B, T, seed=NOISE_SEED):
    """noise_w [B][2][T] first, then noise_z [B][inter][32 T + 64], as the emulator tests draw them."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((B, 2, T)).astype(np.float32),
            rng.standard_normal((B, cfg.inter, 32 * T + 64)).astype(np.float32))


def pairs_of(sp):
    """The (sid, weight) components of a blend entry in their order, or None for an entry that is no blend."""
    if isinstance(sp, dict):
        return [(int(s), float(a)) for s, a in sp.items()]
    if isinstance(sp, (list, tuple)) and len(sp) and isinstance(sp[0], (list, tuple)):
        return [(int(s), float(a)) for s, a in sp]
    return None


def law32(E, sp):
    """g of one `speakers` entry by the law, in f32: the product rounded once, every fmaf rounded once (the f64 sum of an
    exact f32 x f32 product and an f32 addend, rounded to f32 -- a double rounding only on an exact f64 tie)."""
    if sp is None or isinstance(sp, (int, np.integer)):
        return E[int(sp or 0)].copy()
    p = pairs_of(sp)
    if p is None:
        return np.asarray(sp, np.float32).copy()
    g = np.float32(p[0][1]) * E[p[0][0]]
    for s, a in p[1:]:
        g = (np.float64(np.float32(a)) * E[s].astype(np.float64) + g.astype(np.float64)).astype(np.float32)
    return g


def law64(E, sp):
    """(g in f64 from the f32 weights and rows, sum_k |a_k e_k|) of one `speakers` entry; the bound's two ingredients."""
    p = pairs_of(sp)
    if p is None:
        g = law32(E, sp).astype(np.float64)
        return g, np.abs(g)
    g = np.zeros(E.shape[1], np.float64)
    mag = np.zeros(E.shape[1], np.float64)
    for s, a in p:
        t = np.float64(np.float32(a)) * E[s].astype(np.float64)
        g += t
        mag += np.abs(t)
    return g, mag


def check_vector(g, E, sp, what):
    """One utterance's g against the law: exact for a plain id or a vector, under the bound for a blend."""
    g = np.asarray(g, np.float32).reshape(-1)
    if pairs_of(sp) is None:
        assert np.array_equal(g, law32(E, sp)), (what, "not bit for bit")
        return 0.0
    g64, mag = law64(E, sp)
    err = np.abs(g.astype(np.float64) - g64)
    bound = 8 * 2.0 ** -24 * mag
    assert np.all(err <= bound), (what, float(np.max(err / np.maximum(bound, 1e-300))))
    return float(np.max(err / np.maximum(bound, 1e-300)))


def one_row(w, g):
    """The weights with the one-row speaker table g[None]: with sid = 0 the oracle's truth for any g."""
    w1 = dict(w)
    w1["emb_g.weight"] = np.asarray(g, np.float32)[None]
    return w1


_TRUTH = {}


def truth(w, cfg, wkey, ids, scales, nw, nz, speakers):
    """Per utterance the oracle's result on the one-row table of its g (durations, audio, pcm, w in front of the ceil, and
    the durations of the first component's plain speaker); computed once per `wkey` and left unchanged."""
    if wkey not in _TRUTH:
        E = table(w)
        out = []
        for b, sp in enumerate(speakers):
            T = len(ids[b])
            w1 = one_row(w, law32(E, sp))
            o = O.synthesize(w1, cfg, ids[b], scales, nw[b][:, :T], nz[b], sid=0)
            d, wv = O.durations_only(w1, cfg, ids[b], scales, nw[b][:, :T], sid=0, return_w=True)
            p = pairs_of(sp)
            first = O.durations_only(w, cfg, ids[b], scales, nw[b][:, :T], sid=p[0][0] if p else 0)
            out.append({"durations": np.asarray(o["durations"]), "audio": o["audio"], "pcm": o["pcm"], "w": wv, "d_only": d,
                        "first": first})
        _TRUTH[wkey] = out
    return _TRUTH[wkey]


def check_margin(t, what):
    """The condition on the inputs: every oracle w in front of the ceil lies at least W_MARGIN from an integer."""
    dist = min(float(np.min(np.abs(x["w"] - np.round(x["w"])))) for x in t)
    print(f"[{what}] smallest distance of an oracle w from an integer: {dist:.4f}")
    assert dist >= W_MARGIN, (what, dist)


def debug_cases(E, n_utt=64, seed=3):
    """`n_utt` entries whose counts cycle through -1, 0, 1, 8, with a repeated id among the components of every 8-blend, for
    the mixing kernel alone: (speakers, plain sids)."""
    rng = np.random.default_rng(seed)
    nspk, gin = E.shape
    speakers = []
    for b in range(n_utt):
        kind = (-1, 0, 1, 8)[b % 4]
        if kind == -1:
            speakers.append(rng.standard_normal(gin).astype(np.float32))
        elif kind == 0:
            speakers.append(int(rng.integers(nspk)))
        else:
            s = [int(x) for x in rng.integers(nspk, size=kind)]
            if kind == 8:
                s[5] = s[1]
            a = rng.uniform(-1.5, 1.5, size=kind).astype(np.float32)
            speakers.append(list(zip(s, [float(x) for x in a])))
    return speakers


def pcm_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(((a - b) / 32767.0) ** 2))) if a.size else 0.0
