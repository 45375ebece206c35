"""The engine's noise generator (piper_amd/csrc/kernels/rng.h) against a reference written from the algorithm: what
tests/test_rng_emu.py (the kernel emulator) and tests/test_gpu_rng.py (an MI355X) share. numpy only, no device.

The integers. Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), ten rounds of

    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))      M0 = D2511F53  M1 = CD9E8D57
    (k0, k1)         <- (k0 + 9E3779B9, k1 + BB67AE85)                                           after every round

in uint64 arithmetic; KAT holds the three published known-answer vectors of Random123 (kat_vectors, philox4x32_10 rows).

The stream law of include/piper_hip.h (pe_debug_randn): a site's stream is a logical [row][65536] array, element (row, col) is
draw d = row * 65536 + col. Block q = d >> 2 has counter {q lo, q hi, s lo, s hi} with s = 2 * call + site and key {seed lo,
seed hi}; its outputs r[0..3] give elements 4q .. 4q + 3 as (cos, sin) of the pair (r0, r1), then of (r2, r3).

The transform. From a pair (ra, rb) the kernel forms, in f32, u1 = (float(ra) + 1) * 2^-32 in (0, 1] and u2 = float(rb) * 2^-32
in [0, 1]: float() rounds to nearest even like the hardware's conversion, + 1 is inexact only at the top (where it gives 2^32,
u1 = 1), the scaling is exact -- numpy f32 reproduces both bit for bit (uniforms). From THOSE f32 uniforms

    truth       rad = sqrt(-2 ln u1),  t = rad * cos / sin (2 pi u2)                 in f64
    reference   rad = sqrt(f32(-2 ln 2) * log2(u1)),  g = rad * cos / sin (f32(2 pi) * u2)      numpy's own f32 functions

so that what is compared is the three transcendentals, the multiplies and the square root. The normalised error of a set of
draws is E = max |g - t| / rad over the draws with rad > 0; where rad == 0 (u1 == 1.0f, which needs ra >= 2^32 - 128) the
draw itself must be |g| <= 1e-6.

Edge draws. Philox cannot be inverted for a chosen output here, so the endpoints themselves (ra = 0, ra >= 2^32 - 128,
rb = 0) cannot be asked for: edge_draws searches the first 2^22 draws of a (seed, call, site) for the pairs that come closest
-- about 2^-21 from each target -- and the tests report those classes separately."""
import numpy as np

MASK = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))
PITCH = 65536
# (counter, key, output): Random123's kat_vectors for philox4x32 with 10 rounds
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]

CONDITION = 2.0 ** -13        # |g - t| <= CONDITION * max(1, rad) on every element: other integers, another pair order or the
#                               other trig function are O(1) off; any honest f32 transform is below 2^-20
ZERO_RAD = 1e-6               # |g| where rad == 0
EMU_GATE = 1e-6               # E of the emulator (glibc f32 functions): the reference's own 4.1e-7 plus a few f32 ulps
DEVICE_FACTOR = 16            # E of the device <= DEVICE_FACTOR * E of the reference: four bits for hardware units against libm
EDGE_N = 1 << 22              # edge_draws searches this many draws
EDGE_K = 8                    # pairs per class


def philox4x32_10(c, k):
    """c: four, k: two arrays (or ints) of 32-bit words -> the four output words, uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & MASK for x in c]
    k = [np.atleast_1d(np.asarray(x, np.uint64)) & MASK for x in k]
    for _ in range(10):
        p0, p1 = PHILOX_M[0] * c[0], PHILOX_M[1] * c[2]            # 32 x 32 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + PHILOX_W[0]) & MASK, (k[1] + PHILOX_W[1]) & MASK]
    return c


def stream(seed, call, site, row, col0, n):
    """The integers of draws (row, col0) .. + n of a site's stream: (ra, rb, trig) per draw -- the pair the draw is made of
    (uint64 arrays of 32-bit values) and 0 for its cosine, 1 for its sine."""
    seed, s = int(seed) % 2 ** 64, (2 * int(call) + int(site)) % 2 ** 64
    d0 = int(row) * PITCH + int(col0)
    q0, q1 = d0 >> 2, (d0 + int(n) - 1) >> 2
    q = np.uint64(q0) + np.arange(q1 - q0 + 1, dtype=np.uint64)
    r = philox4x32_10((q & MASK, q >> np.uint64(32), s & 0xFFFFFFFF, s >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    r = np.stack([np.broadcast_to(x, q.shape) for x in r], axis=1)              # [blocks][4]
    ra, rb = np.repeat(r[:, 0::2].reshape(-1), 2), np.repeat(r[:, 1::2].reshape(-1), 2)       # per element of the blocks
    lo = d0 - 4 * q0
    trig = (np.arange(ra.size) & 1).astype(np.int64)
    return ra[lo:lo + n], rb[lo:lo + n], trig[lo:lo + n]


def uniforms(ra, rb):
    """The kernel's f32 uniforms, bit for bit."""
    one, sc = np.float32(1.0), np.float32(2.0 ** -32)
    return (ra.astype(np.float32) + one) * sc, rb.astype(np.float32) * sc


def transform(ra, rb, trig):
    """(t, rad, g32): the f64 truth, its radius, and the f32 reference (module docstring)."""
    u1, u2 = uniforms(ra, rb)
    a, b = u1.astype(np.float64), u2.astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(a))
    ang = 2.0 * np.pi * b
    t = rad * np.where(trig == 1, np.sin(ang), np.cos(ang))
    rad32 = np.sqrt(np.float32(-1.3862943611198906) * np.log2(u1))
    ang32 = np.float32(6.283185307179586) * u2
    g32 = rad32 * np.where(trig == 1, np.sin(ang32), np.cos(ang32))
    assert g32.dtype == np.float32 and rad32.dtype == np.float32
    return t, rad, g32


def truth(seed, call, site, row, col0, n):
    return transform(*stream(seed, call, site, row, col0, n))


def errors(g, t, rad):
    """(E, e, z): max |g - t| / rad over rad > 0, max |g - t|, max |g| over rad == 0 (0.0 where there is none)."""
    d = np.abs(np.asarray(g, np.float64) - t)
    pos = rad > 0
    E = float(np.max(d[pos] / rad[pos])) if pos.any() else 0.0
    z = float(np.max(np.abs(np.asarray(g, np.float64)[~pos]))) if (~pos).any() else 0.0
    return E, float(np.max(d)) if d.size else 0.0, z


def check(g, t, rad, gate, what):
    """Every element under the condition, the zero-radius draws under theirs, E under `gate`; the figures are printed first."""
    g = np.asarray(g)
    assert g.dtype == np.float32 and g.shape == t.shape, (what, g.dtype, g.shape, t.shape)
    assert np.all(np.isfinite(g)), (what, "not finite", np.flatnonzero(~np.isfinite(g))[:8])
    E, e, z = errors(g, t, rad)
    print(f"{what}: n {g.size} E {E:.3e} e {e:.3e} gate {gate:.3e} max |t| {float(np.max(np.abs(t))):.2f}")
    bad = np.flatnonzero(np.abs(g.astype(np.float64) - t) > CONDITION * np.maximum(1.0, rad))
    assert bad.size == 0, (what, "not the documented stream", bad.size, bad[:8], g[bad[:8]], t[bad[:8]])
    assert z <= ZERO_RAD, (what, "rad == 0", z)
    assert E <= gate, (what, E, gate)
    return E, e


_REFERENCE_E = {}


def reference_error(seed=2026, call=1, site=0, n=EDGE_N):
    """E of the f32 reference over the first n draws of (seed, call, site): what the device's gate is a multiple of. A window of
    a few draws is held to this figure too -- the maximum over a handful of draws is no estimate of the reference's error."""
    key = (seed, call, site, n)
    if key not in _REFERENCE_E:
        t, rad, g32 = truth(seed, call, site, 0, 0, n)
        _REFERENCE_E[key] = errors(g32, t, rad)[0]
    return _REFERENCE_E[key]


# ---- edge draws
EDGE_CLASSES = ("u1 smallest", "u1 nearest 1", "u2 nearest 0", "u2 nearest 0.25", "u2 nearest 0.5", "u2 nearest 0.75", "u2 largest")


def edge_draws(seed, call, site, n=EDGE_N, k=EDGE_K):
    """{class: positions} within draws [0, n) of (seed, call, site): both draws (cosine and sine) of the k pairs that come
    closest to each edge, chosen on the integers (the f32 uniforms tie near 1). From the reference alone."""
    ra, rb, _ = stream(seed, call, site, 0, 0, n)
    a, b = ra[0::2].astype(np.int64), rb[0::2].astype(np.int64)                   # one entry per pair
    keys = {"u1 smallest": a, "u1 nearest 1": -a, "u2 nearest 0": b, "u2 nearest 0.25": np.abs(b - 2 ** 30),
            "u2 nearest 0.5": np.abs(b - 2 ** 31), "u2 nearest 0.75": np.abs(b - 3 * 2 ** 30), "u2 largest": -b}
    out = {}
    for name in EDGE_CLASSES:
        p = np.sort(np.argsort(keys[name], kind="stable")[:k])
        out[name] = np.stack([2 * p, 2 * p + 1], axis=1).reshape(-1)
    return out


def describe_edges(seed, call, site, edges):
    """One line per class: the extreme uniforms the finder produced (profiles/rng_truth.md)."""
    ra, rb, _ = stream(seed, call, site, 0, 0, EDGE_N)
    u1, u2 = uniforms(ra, rb)
    lines = []
    for name in EDGE_CLASSES:
        p = edges[name]
        lines.append(f"{name}: u1 in [{float(u1[p].min()):.9g}, {float(u1[p].max()):.9g}] u2 in [{float(u2[p].min()):.9g}, "
                     f"{float(u2[p].max()):.9g}] draws {p[::2].tolist()}")
    return lines


# ---- the stream law: the windows both targets walk through
WINDOW_N = (1, 2, 3, 5, 1023, 1025, 65535, 65537)      # ends inside a block, a row's second workgroup, the seam of two rows
WINDOW_ROWS = (0, 1, 262143, 262144, 262145)           # q = row * 16384 crosses 2^32: the counter's second word
WINDOW_CALLS = (2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5)     # s = 2 * call + site crosses 2^32: the counter's fourth word
WINDOW_SEEDS = (1, 2 ** 32, 2 ** 32 + 1, 0xDEADBEEF12345678)      # the key's second word


def windows():
    """(seed, call, site, row, n): every n at every row under the last seed and call (all high words in use) and under the
    plain (1, 1); then two sizes at two rows under every call (and 1) and every seed."""
    out = []
    for n in WINDOW_N:
        for row in WINDOW_ROWS:
            out.append((WINDOW_SEEDS[-1], WINDOW_CALLS[-1], (n + row) & 1, row, n))
    for n in WINDOW_N:
        out.append((1, 1, n & 1, 0, n))
    for seed in WINDOW_SEEDS:
        for call in (1,) + WINDOW_CALLS:
            for row in (0, 262144):
                for n in (5, 1025):
                    out.append((seed, call, (row >> 18) ^ (n & 1) ^ (call & 1), row, n))
    return out


def check_windows(eng, gate, what):
    """debug_randn of every window against stream() plus the transform. Returns the worst E."""
    worst, seed_now = 0.0, None
    for seed, call, site, row, n in windows():
        if seed != seed_now:
            eng.set_seed(seed)
            seed_now = seed
        g = eng.debug_randn(site, call, n, row=row)
        t, rad, _ = truth(seed, call, site, row, 0, n)
        E, _ = check(g, t, rad, gate, f"[{what} seed {seed:#x} call {call} site {site} row {row} n {n}]")
        worst = max(worst, E)
    return worst


# ---- the product path: what an engine drew in its last call
def check_engine_noise(eng, cfg, seed, call, lens, gate, what, sites=(0, 1)):
    """noise_w / noise_z of every utterance of the engine's last call: bit-equal to debug_randn at (seed, call) and under the
    gates against the truth. Rows are 2 b + c and inter b + c; only an utterance's own ids / frames are read (debug_tensor
    returns no padding column). Returns the frame counts (with site 1 among `sites`)."""
    assert eng.rng_calls == call, (what, eng.rng_calls, call)
    frames = []
    for b, T in enumerate(lens):
        got = []
        if 0 in sites:
            nw = eng.debug_tensor("noise_w", b)
            assert nw.shape == (2, T), (what, b, nw.shape)
            got.append((0, nw, 2))
        if 1 in sites:
            nz = eng.debug_tensor("noise_z", b)
            assert nz.shape[0] == cfg.inter and nz.shape[1] >= 1, (what, b, nz.shape)
            frames.append(nz.shape[1])
            got.append((1, nz, cfg.inter))
        for site, x, ch in got:
            t = np.empty(x.shape, np.float64)
            rad = np.empty(x.shape, np.float64)
            for c in range(ch):
                assert np.array_equal(x[c], eng.debug_randn(site, call, x.shape[1], row=ch * b + c)), (what, b, site, c)
                t[c], rad[c], _ = truth(seed, call, site, ch * b + c, 0, x.shape[1])
            check(np.ascontiguousarray(x).reshape(-1), t.reshape(-1), rad.reshape(-1), gate, f"[{what} call {call} utt {b} site {site}]")
    return frames


SCALES = (0.667, 1.0, 0.8)
DRAW_KERNELS = ("embed_kernel", "randn_kernel", "regulate_kernel")
DEFAULT_SEED = 1234          # include/piper_hip.h: pe_set_seed


def check_group(lib, monkeypatch, vname, gate, what, ids_len=7):
    """EngineGroup(blob, [0, 0]) with no set_seed, twice: on two texts of equal length, one per member, the members' local
    utterance 0 must not share its noise, and member i's noise is the reference's at seed DEFAULT_SEED + i."""
    from piper_amd import weights as W
    from piper_amd.group import EngineGroup
    cfg = W.preset(vname)
    blob = W.pack_blob(cfg, W.synthetic_weights(cfg, 1234))
    ids = [W.synthetic_phoneme_ids(ids_len, 90 + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(2)]
    monkeypatch.setenv("PIPER_HIP_GROUP_COALESCE", "0")          # both members take part in a call of two utterances
    monkeypatch.setenv("PIPER_HIP_DEBUG_KEEP", "1")
    for attempt in range(2):
        grp = EngineGroup(blob, [0, 0]) if lib is None else EngineGroup(blob, [0, 0], lib=lib)
        try:
            grp.synthesize_batch(ids, SCALES)
            assert sorted(grp.assignment(2)) == [0, 1]
            members = [grp.engine(i) for i in range(2)]
            noise = [(m.debug_tensor("noise_w", 0), m.debug_tensor("noise_z", 0)) for m in members]
            assert noise[0][0].shape == noise[1][0].shape == (2, ids_len)
            F = min(noise[0][1].shape[1], noise[1][1].shape[1])
            assert not np.array_equal(noise[0][0], noise[1][0]), (what, attempt, "both members drew the same duration noise")
            assert not np.array_equal(noise[0][1][:, :F], noise[1][1][:, :F]), (what, attempt, "both members drew the same prior noise")
            for i, m in enumerate(members):
                check_engine_noise(m, cfg, DEFAULT_SEED + i, 1, [ids_len], gate, f"{what} group {attempt} member {i}")
        finally:
            grp.close()


def product_calls(eng, cfg, seed, ids, gate, what, scales=SCALES, runs=4, graph=None):
    """Calls 1 .. runs of a fresh engine with its own noise at both sites, each through check_engine_noise, and one more
    under the level-2 profile (a profiled call is never a graph), checked alike. `graph` says how calls 2 .. runs must have
    been issued: "spec" (the whole utterance as one graph), "two" (graphs, none speculative), "none" (nothing captured),
    None (not asserted: the emulator has no graphs); with graphs, one of the calls must have replayed one without capturing.
    Returns ({kernel name: launches} of the profiled call, the frame counts of the last call)."""
    assert eng.rng_calls == 0, (what, "not a fresh engine")
    eng.set_seed(seed)
    lens = [len(s) for s in ids]
    replays = 0
    for call in range(1, runs + 1):
        s0, g0 = eng.speculation_stats, eng.graph_stats
        eng.synthesize_batch(ids, scales)
        s1, g1 = eng.speculation_stats, eng.graph_stats
        print(f"[{what}] call {call}: speculation {s0} -> {s1} graphs {g0} -> {g1}")
        if graph is not None and call >= 2:
            if graph == "spec":
                assert s1[0] == s0[0] + 1 and s1[1] == s0[1], (what, call, "not the one whole-utterance graph", s0, s1)
            else:
                assert s1 == s0, (what, call, graph, s0, s1)
            assert (g1[0] == 0) == (graph == "none"), (what, call, graph, g1)
        replays += call >= 2 and g1[0] > 0 and g1[1] == g0[1]
        check_engine_noise(eng, cfg, seed, call, lens, gate, what)
    # (the engine's own noise moves the frame count from call to call, and with it now and then the frame bucket of the graph:
    # which calls replay is a matter of the seed, that one does is asserted)
    assert graph in (None, "none") or replays >= 1, (what, "no call replayed a captured graph")
    eng.profile_enable(2)
    eng.profile_reset()
    try:
        eng.synthesize_batch(ids, scales)
        names = {row["name"]: int(row["launches"]) for row in eng.profile()[5:] if row["launches"]}
    finally:
        eng.profile_enable(0)
    frames = check_engine_noise(eng, cfg, seed, runs + 1, lens, gate, what + " profiled")
    print(f"[{what}] frames {frames} draw kernels: { {k: v for k, v in names.items() if k in DRAW_KERNELS} }")
    return names, frames
