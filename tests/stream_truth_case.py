"""The chunked decode against f64 truths, window edges and halo included: what tests/test_gpu_stream_truth.py (an MI355X) and
tests/test_stream_truth_emu.py (the kernel emulator) share -- the three ways to play a stream, and every check as a function.

The three paths: the one-utterance stream (pe_stream_next, stage W: window_copy_kernel), the batch stream in lock step
(pe_stream_next_batch, stage V: window_gather_kernel, chunk_peak_kernel, chunk_pcm_kernel) and the stream pool (stage P, the same
kernels on resident rows that stream_adopt_kernel filled). Every engine runs with PIPER_HIP_DEBUG_KEEP=1 and
PIPER_HIP_DEBUG_POISON=1: a window column read without having been written is a NaN in the output, and a NaN fails every gate.

The truth of a chunk. The latent is the ENGINE'S OWN (debug_tensor "z" once the stream has begun, "pool_z" for a pool row), so
the front half's and the flow's error are not in any figure here. For an utterance of F frames, the voice's halo h and a chunk of
frames [f0, f1) the window is restated here, not read from the engine:

    a = max(0, f0 - h)      e = min(F, f1 + h)

    t64_full   the f64 generator on the whole z (with the speaker's row)        truth of the chunk: samples [f0 hop, f1 hop)
    f32 ref    the oracle's f32 generator on z[:, a:e], trimmed to the chunk
    precondition, asserted before any engine figure is looked at: the f64 generator on z[:, a:e], trimmed, equals the slice of
    t64_full within 1e-12 max |t64_full| (first, middle and last chunk of every utterance). It is what makes ONE unchunked f64
    decode the truth of every chunking.

    per utterance, pooled over its chunks   e_hip <= K e_ref + fl  and  r_hip <= K r_ref      fl = 2^-23 max |t64_full|
    per chunk (a 256-sample chunk has too few samples for a ratio of its own)   e_hip <= K (the utterance's pooled e_ref) + fl
    per chunk   the int16 is oracle.audio_float_to_int16 of the chunk's own floats, bit for bit; min(asked, F - f0) hop samples

K = GATES[target]["audio"] of tests/one_utterance_truth_case.py: 8, "two f32 summation orders". profiles/stream_truth.md has the
measured figures.

The halo check, which the gates cannot do: a window one frame short changes a chunk by 5e-7, below 8 e_ref. For a ResBlock2
voice let A be the f64 truth of a chunk, B the f64 decode of the window with one halo frame fewer on one side, d = B - A, and over
all chunks of a case with a full halo on that side

    s(x) = sum <x - A, d> / sum <d, d>          0 for an exact window, 1 for a window one frame short

First the f32 reference alone must give |s(f32 of A)| <= 1/16 and s(f32 of B) in [0.9, 1.1] on at least 6 chunks (the case can
tell the two apart); then the engine's chunks must give |s| <= 0.5. An engine whose rounding error is the full 8 times the
reference's stays at or below 0.5. For the ResBlock1 voice the 13th and 14th frame weigh 1e-11: no f32 check is possible, the
emulator file asserts in f64 that one frame less changes nothing (the bound is one frame generous).

The compared call is the production one (as one_utterance_truth_case.run): a first play with other ids and other noise of the
same lengths (repeated until it captures nothing), so that no buffer of it can pass for the second's; the figures are the second play's, during which graph_stats
must show that nothing was captured; a third play under the level-2 profile must reproduce every chunk bit for bit and names the
kernels. The emulator has no graphs: one profiled play. The noise of both sites is injected, so the three plays of a stream see
the same latent; frame counts are forced through the timing plan where the path has a timed entry (batch stream, pool join) and
picked on the CPU oracle otherwise (pick_scale, under ORACLE_MARGIN).

Out of scope, tested elsewhere: converted output rates, the running and fixed stream gains, loudness, the limiter and the seeds."""
import ctypes as C

import numpy as np
import torch

import one_utterance_truth_case as U
import stream_pool_case as P
from piper_amd import weights as W
from piper_amd.engine import Timing

O = U.O
ENV = {"PIPER_HIP_DEBUG_POISON": 1}
PRECONDITION = 1e-12
MIN_HALO_CHUNKS = 6
STAGE = {"W": {"window_copy_kernel"}, "V": {"window_gather_kernel", "chunk_peak_kernel", "chunk_pcm_kernel"},
         "P": {"window_gather_kernel", "chunk_peak_kernel", "chunk_pcm_kernel", "stream_adopt_kernel"}}

ROWS = []        # (target, voice, path, case, mode, utterance, F, chunks, e_hip, e_ref, r_hip, r_ref, worst chunk ratio, precondition)
HALO = []        # (target, voice, path, case, side, chunks, s of f32 on A, s of f32 on B, s of the engine)
KERNELS = {}     # (target, voice, path, case) -> sorted kernel names
_WEIGHTS = {}


class Utt(P.Listener):
    """One utterance of a stream: its inputs, and what the play left -- F, the engine's latent z [C][F], the delivered chunks
    with the size that was asked for each and the call that delivered it."""

    def __init__(self, name, ids, scales, sid, nw, nz, forced=None):
        super().__init__(name, ids, scales, sid, nw, nz)
        self.forced = None if forced is None else np.asarray(forced, np.int32)
        self.z, self.asked, self.calls = None, [], []

    def fresh(self):
        return Utt(self.name, self.ids, self.scales, self.sid, self.nw, self.nz, self.forced)

    def other(self, top):
        """Other ids and other noise of the same lengths (reversed; the next id and negated noise for a palindrome)."""
        ids = self.ids[::-1].copy()
        nw = self.nw[:, ::-1]
        if np.array_equal(ids, self.ids):
            ids, nw = (self.ids + 1) % top, -self.nw
        return Utt(self.name + "'", ids, self.scales, self.sid, nw, -self.nz[:, ::-1], self.forced)


def spread(T, F):
    """F frames over T ids, as evenly as integers allow (ids of 0 frames when F < T)."""
    d = np.full(T, F // T, np.int32)
    d[:F % T] += 1
    return d


def utt(cfg, name, T, index, seed, F=None, sid=None, scales=U.SCALES, cols=None):
    """T synthetic ids with Gaussian noise for both sites; F given: every id's duration forced, F frames in all."""
    ids = W.synthetic_phoneme_ids(T, index, id_max=min(cfg.n_vocab - 1, 129))
    rng = np.random.default_rng(seed)
    nw = rng.standard_normal((2, T)).astype(np.float32)
    nz = rng.standard_normal((cfg.inter, cols or (F + 8 if F else 48 * T + 64))).astype(np.float32)
    return Utt(name, ids, scales, sid, nw, nz, None if F is None else spread(T, F))


def pick_scale(vname, u, F, wseed=1234):
    """The length_scale, a multiple of 0.01 and the nearest to 1, at which the CPU oracle gives utterance u exactly F frames
    with every duration ORACLE_MARGIN (relative) from an integer before the ceil; returns u with that scale. logw does not
    depend on the scale, so one run of the duration predictor serves the search; the pick is then verified by a run of its own."""
    cfg, w = U.voice(vname, wseed)
    wt = weights_as(vname, wseed, torch.float32)
    sc = list(u.scales)
    _, w1 = O.durations_only(wt, cfg, u.ids, (sc[0], 1.0, sc[2]), u.nw, sid=u.sid, return_w=True)
    for ls in sorted(np.round(np.arange(0.2, 4.0, 0.01), 2), key=lambda v: abs(v - 1.0)):
        v = w1.astype(np.float32) * np.float32(ls)
        if int(np.ceil(v).sum()) != F or np.min(np.abs(v - np.round(v)) / np.maximum(1.0, v)) < 4 * U.ORACLE_MARGIN:
            continue
        d, wv = O.durations_only(wt, cfg, u.ids, (sc[0], float(ls), sc[2]), u.nw, sid=u.sid, return_w=True)
        dist = float(np.min(np.abs(wv - np.round(wv)) / np.maximum(1.0, wv)))
        if int(d.sum()) == F and dist >= U.ORACLE_MARGIN:
            print(f"[{vname} {u.name}] length_scale {ls:.2f}: {F} frames, the oracle's durations stay {dist:.2e} from an integer")
            return Utt(u.name, u.ids, (sc[0], float(ls), sc[2]), u.sid, u.nw, u.nz, None)
    raise AssertionError((vname, u.name, F, "no length_scale gives this frame count under the margin"))


# ---- the generator in a chosen precision
def weights_as(vname, wseed, dtype):
    if (vname, wseed, dtype) not in _WEIGHTS:
        _WEIGHTS[vname, wseed, dtype] = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in U.voice(vname, wseed)[1].items()}
    return _WEIGHTS[vname, wseed, dtype]


def generate(vname, wseed, dtype, z, sid):
    """oracle.stage_truths' stage G on z [C][n] in `dtype` (the weights converted once per voice)."""
    cfg, _ = U.voice(vname, wseed)
    return O.stage_truths(weights_as(vname, wseed, dtype), cfg, [0], (1.0, 1.0, 1.0), None, None, {"z": np.ascontiguousarray(z)},
                          sid=sid, dtype=dtype, stages="G")["audio"]


# ---- the three plays. Each fills u.F, u.z, u.chunks, u.asked and u.calls of its utterances and returns the halo.
def play_one(eng, u, asks):
    """pe_stream_begin / pe_stream_next called directly: chunk k asks for asks[min(k, last)] frames."""
    lib, h = eng._lib, eng._h
    ids = np.ascontiguousarray(u.ids, np.int64)
    sc = (C.c_float * 3)(*u.scales)
    keep = []
    nref = eng._noise(u.nw[None], u.nz[None], keep)
    frames, halo = C.c_int32(), C.c_int32()
    eng._check(lib.pe_stream_begin(h, ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size, sc, -1 if u.sid is None else int(u.sid),
                                   nref, C.byref(frames), C.byref(halo)))
    u.F, u.z = frames.value, eng.debug_tensor("z", 0)
    k = 0
    while True:
        a, p, n = C.POINTER(C.c_float)(), C.POINTER(C.c_int16)(), C.c_int64()
        ask = int(asks[min(k, len(asks) - 1)])
        eng._check(lib.pe_stream_next(h, ask, C.byref(a), C.byref(p), C.byref(n)))
        if n.value == 0:
            return halo.value
        u.chunks.append((np.ctypeslib.as_array(a, (n.value,)).copy(), np.ctypeslib.as_array(p, (n.value,)).copy()))
        u.asked.append(ask)
        u.calls.append(k)
        k += 1
        assert k < 400


def _timing(utts):
    return None if utts[0].forced is None else Timing(durations=[u.forced for u in utts])


def play_batch(eng, utts, chunk):
    """Engine.stream_batch in lock step; `chunk`: an int or k -> frames. A row that has finished delivers nothing."""
    gen = eng.stream_batch([u.ids for u in utts], np.array([u.scales for u in utts], np.float32),
                           sids=None if utts[0].sid is None else [u.sid for u in utts], chunk_frames=chunk,
                           noise_w=P.pad_stack([u.nw for u in utts]), noise_z=P.pad_stack([u.nz for u in utts]), timing=_timing(utts))
    done = np.zeros(len(utts), np.int64)
    for k, item in enumerate(gen):
        assert k < 400
        ask = int(chunk(k)) if callable(chunk) else int(chunk)
        if k == 0:
            for b, u in enumerate(utts):
                u.F, u.z = int(eng.stream_frames[b]), eng.debug_tensor("z", b)
        for b, ((a, p), u) in enumerate(zip(item, utts)):
            if done[b] == u.F:
                assert p.size == 0 and a.size == 0, (u.name, k, "a finished row delivered samples")
                continue
            assert p.size and a.shape == p.shape, (u.name, k)
            u.chunks.append((a.copy(), p.copy()))
            u.asked.append(ask)
            u.calls.append(k)
        done = eng.stream_frames_done.astype(np.int64)
    assert all(done[b] == u.F for b, u in enumerate(utts)), (done, [u.F for u in utts])
    return eng.stream_halo


def pool_join(eng, pool, utts, held=None):
    """A join; then every newcomer's resident row is its latent bit for bit on [0, F) and exactly zero behind it (`held`: the
    frames the slot's last tenant had, which must have left something there). The truth of a pool chunk comes from that row."""
    before = {s: eng.debug_tensor("pool_z", s) for s in (held or {})}
    slots = pool.join([u.ids for u in utts], np.array([u.scales for u in utts], np.float32),
                      sids=None if utts[0].sid is None else [u.sid for u in utts], noise_w=P.pad_stack([u.nw for u in utts]),
                      noise_z=P.pad_stack([u.nz for u in utts]), timing=_timing(utts))
    frames = pool.frames
    for j, (u, s) in enumerate(zip(utts, slots)):
        u.slot, u.F = s, int(frames[s])
        row, z = eng.debug_tensor("pool_z", s), eng.debug_tensor("z", j)
        assert z.shape == (row.shape[0], u.F) and row.shape[1] >= u.F, (u.name, z.shape, row.shape)
        assert np.array_equal(row[:, :u.F], z), (u.name, "the resident row is not the newcomer's latent")
        assert not np.any(row[:, u.F:]), (u.name, "the resident row is not zero behind the newcomer's frames")
        if held and s in held:
            assert held[s] > u.F and np.all(np.abs(before[s][:, u.F:held[s]]).max(axis=0) > 0), (u.name, "the old tenant left nothing")
        u.z = row[:, :u.F].copy()
    return slots


def play_pool(eng, pool, first_three, newcomer, leaver, first, chunk, leave_after=3):
    """Three listeners join together with a short first chunk each (per_slot); after `leave_after` calls first_three[leaver]
    hangs up in mid-stream and the newcomer, a shorter utterance, takes its slot, again with a short first chunk; then to the end."""
    assert pool.free_slots == list(range(pool.slots))
    assert pool_join(eng, pool, first_three) == [0, 1, 2]
    on = {u.slot: u for u in first_three}
    pending = {s: first for s in on}
    calls = 0
    while True:
        before = pool.frames_done
        out = pool.next(chunk, per_slot=pending or None)
        done = pool.frames_done
        if not out:
            assert np.array_equal(done, before)
            break
        for s, u in on.items():
            got = int(done[s] - before[s])
            if u.left or before[s] == u.F:
                assert s not in out and got == 0, (calls, u.name, "a row with nothing to deliver delivered")
                continue
            a, p = out[s]
            assert got > 0 and p.size == got * eng.hop and a.shape == p.shape, (calls, u.name)
            u.chunks.append((a.copy(), p.copy()))
            u.asked.append(pending.get(s, chunk))
            u.calls.append(calls)
        pending = {}
        calls += 1
        assert calls < 400
        if calls == leave_after:
            gone = first_three[leaver]
            assert 0 < done[gone.slot] < gone.F, (gone.name, "not in mid-stream")
            pool.leave(gone.slot)
            gone.left = True
            assert pool.free_slots[0] == gone.slot
            assert pool_join(eng, pool, [newcomer], held={gone.slot: gone.F}) == [gone.slot]
            on[gone.slot] = newcomer
            pending = {gone.slot: first}
    assert newcomer.slot is not None and pool.free_slots == list(range(pool.slots))
    return pool.halo


def compared(eng, play, utts, emu):
    """The compared play (module docstring): play(list of fresh Utt) -> halo. Returns (utterances of the compared play, halo,
    {kernel name: launches} of the profiled repeat)."""
    def profiled():
        rep = [u.fresh() for u in utts]
        eng.profile_enable(2)
        eng.profile_reset()
        try:
            halo = play(rep)
            names = {row["name"]: int(row["launches"]) for row in eng.profile()[5:] if row["launches"]}
        finally:
            eng.profile_enable(0)
        return rep, halo, names

    if emu:
        return profiled()
    top = 1 + max(int(u.ids.max()) for u in utts)
    for _ in range(3):          # until a play captures nothing: growing a workspace in mid-play drops the graphs captured before it
        c0 = eng.graph_stats[1]
        others = [u.other(top) for u in utts]
        play(others)
        if eng.graph_stats[1] == c0:
            break
    got = [u.fresh() for u in utts]
    g0 = eng.graph_stats
    halo = play(got)
    g1 = eng.graph_stats
    assert g1[0] > 0 and g1[1] == g0[1], ("the compared play captured a graph: it was not the replay of a warm engine", g0, g1)
    for u, o in zip(got, others):          # the first play left other values in the latent, and with it in every window
        assert o.z.shape != u.z.shape or not np.array_equal(o.z, u.z), (u.name, "the first play's latent")
    rep, halo2, names = profiled()
    assert halo2 == halo
    for u, r in zip(got, rep):          # the names are the repeat's: it must be the same play
        assert r.F == u.F and np.array_equal(r.z, u.z) and len(r.chunks) == len(u.chunks) and r.asked == u.asked, u.name
        for k, ((a, p), (ra, rp)) in enumerate(zip(u.chunks, r.chunks)):
            assert np.array_equal(a, ra) and np.array_equal(p, rp), (u.name, k, "the profiled repeat gave other bits")
    return got, halo, names


# ---- the checks
def windows(u, h, hop):
    """(f0, f1, a, e) per delivered chunk by the documented rule; the sizes must be exactly min(asked, F - f0) hop samples."""
    out, f0 = [], 0
    for k, ((a, p), ask) in enumerate(zip(u.chunks, u.asked)):
        f1 = min(u.F, f0 + ask)
        assert f0 < u.F and a.size == p.size == (f1 - f0) * hop, (u.name, k, a.size, p.size, f0, f1, ask)
        assert a.dtype == np.float32 and p.dtype == np.int16, (u.name, k)
        out.append((f0, f1, max(0, f0 - h), min(u.F, f1 + h)))
        f0 = f1
    assert f0 == u.F or u.left, (u.name, f0, u.F, "the stream ended early")
    return out


def check_utterance(target, vname, path, case, u, h, hop, mode="f32", wseed=1234, K="gate"):
    """Precondition, per-chunk table, per-chunk and pooled gates, int16 rule and sizes of one utterance; returns (the pooled
    figures, one record per chunk for the halo check). K: None = printed, gated by the caller (a split matrix mode)."""
    what = f"[{target} {vname} {path} {case} {mode} {u.name} F={u.F}]"
    assert u.z.shape[1] == u.F and u.chunks, what
    K = U.GATES[target]["audio"] if K == "gate" else K
    win = windows(u, h, hop)
    full = generate(vname, wseed, torch.float64, u.z, u.sid)
    assert full.shape == (u.F * hop,), what
    peak = float(np.max(np.abs(full)))
    fl = 2.0 ** -23 * peak
    # the precondition, before any engine figure: the f64 window decode IS the slice of the one unchunked f64 decode
    pre = 0.0
    for k in sorted({0, len(win) // 2, len(win) - 1}):
        f0, f1, a, e = win[k]
        w64 = generate(vname, wseed, torch.float64, u.z[:, a:e], u.sid)[(f0 - a) * hop:(f1 - a) * hop]
        pre = max(pre, float(np.max(np.abs(w64 - full[f0 * hop:f1 * hop]))))
    print(f"{what} precondition: max |f64 window - f64 whole| {pre:.2e} (bound {PRECONDITION * peak:.2e})")
    assert pre <= PRECONDITION * peak, (what, pre, peak)
    recs = []
    for k, (f0, f1, a, e) in enumerate(win):
        r32 = generate(vname, wseed, torch.float32, u.z[:, a:e], u.sid)[(f0 - a) * hop:(f1 - a) * hop]
        recs.append(dict(u=u, k=k, f0=f0, f1=f1, a=a, e=e, hip=u.chunks[k][0], A=full[f0 * hop:f1 * hop], r32=r32))
    fig = U.figures(np.concatenate([r["hip"] for r in recs]), np.concatenate([r["A"] for r in recs]),
                    np.concatenate([r["r32"] for r in recs]))
    fig["fl"] = fl
    bad, worst = [], 0.0
    for r in recs:
        eh, er = float(np.max(np.abs(r["hip"] - r["A"]))), float(np.max(np.abs(r["r32"] - r["A"])))
        ratio = eh / max(fig["e_ref"], 1e-300)
        worst = max(worst, ratio) if eh == eh else float("nan")
        print(f"{what} chunk {r['k']} call {u.calls[r['k']]} [{r['f0']}, {r['f1']}) window [{r['a']}, {r['e']}): e_hip {eh:.3e} e_ref {er:.3e} "
              f"e_hip / pooled e_ref {ratio:.2f}")
        if K is not None and not eh <= K * fig["e_ref"] + fl:
            bad.append((r["k"], eh))
    print(f"{what} pooled over {len(recs)} chunks: e_hip {fig['e_hip']:.3e} e_ref {fig['e_ref']:.3e} ratio "
          f"{fig['e_hip'] / max(fig['e_ref'], 1e-300):.2f} | r_hip {fig['r_hip']:.3e} r_ref {fig['r_ref']:.3e} ratio "
          f"{fig['r_hip'] / max(fig['r_ref'], 1e-300):.2f} | fl {fl:.2e} K {K}")
    ROWS.append((target, vname, path, case, mode, u.name, u.F, len(recs), fig["e_hip"], fig["e_ref"], fig["r_hip"], fig["r_ref"], worst, pre / peak))
    assert not bad, (what, "chunks over K * pooled e_ref + fl", K, fig["e_ref"], fl, bad)
    if K is not None:
        assert fig["e_hip"] <= K * fig["e_ref"] + fl and fig["r_hip"] <= K * fig["r_ref"], (what, K, fig)
    for r in recs:
        assert np.array_equal(O.audio_float_to_int16(r["hip"]), u.chunks[r["k"]][1]), (what, r["k"], "int16 of the chunk's own floats")
    return fig, recs


def check_halo(target, vname, path, case, recs, h, hop, wseed=1234):
    """The halo check per side over the chunk records of a case: the reference's two conditions first, then the engine's."""
    out = {}
    for side in ("left", "right"):
        use = [r for r in recs if (r["f0"] - h >= 0 if side == "left" else r["f1"] + h <= r["u"].F)]
        num = {"A32": 0.0, "B32": 0.0, "hip": 0.0}
        den = 0.0
        for r in use:
            u, a, e = r["u"], r["a"], r["e"]
            assert (a == r["f0"] - h) if side == "left" else (e == r["f1"] + h)
            a, e = (a + 1, e) if side == "left" else (a, e - 1)
            cut = slice((r["f0"] - a) * hop, (r["f1"] - a) * hop)
            B = generate(vname, wseed, torch.float64, u.z[:, a:e], u.sid)[cut]
            B32 = generate(vname, wseed, torch.float32, u.z[:, a:e], u.sid)[cut]
            d = B - r["A"]
            den += float(d @ d)
            for key, x in (("A32", r["r32"]), ("B32", B32), ("hip", r["hip"])):
                num[key] += float((x.astype(np.float64) - r["A"]) @ d)
        s = {k: v / max(den, 1e-300) for k, v in num.items()}
        print(f"[{target} {vname} {path} {case}] halo, {side}: {len(use)} chunks, sum <d, d> {den:.3e}, s(f32 of A) {s['A32']:+.4f} "
              f"s(f32 of B) {s['B32']:.4f} s(engine) {s['hip']:+.4f}")
        HALO.append((target, vname, path, case, side, len(use), s["A32"], s["B32"], s["hip"]))
        out[side] = (len(use), s)
    for side, (n, s) in out.items():
        assert n >= MIN_HALO_CHUNKS, (case, side, n, "too few chunks with a full halo")
        assert abs(s["A32"]) <= 1 / 16 and 0.9 <= s["B32"] <= 1.1, (case, side, s, "the f32 reference cannot tell the two windows apart")
    for side, (n, s) in out.items():
        assert abs(s["hip"]) <= 0.5, (case, side, s, "the engine's window is not the documented one")
    return out


def check_case(target, vname, path, case, utts, h, hop, names, wanted=(), halo=True, mode="f32", wseed=1234, K="gate"):
    """Every utterance of a compared play, the halo check over all their chunks (halo=False: the caller pools the returned chunk
    records of several plays into one check_halo), and the kernels the case is there for. Returns (figures, chunk records)."""
    cfg, _ = U.voice(vname, wseed)
    KERNELS[target, vname, path, case] = sorted(names)
    print(f"[{target} {vname} {path} {case} {mode}] halo {h}, kernels: {sorted(names)}")
    figs, recs = [], []
    for u in utts:
        f, r = check_utterance(target, vname, path, case, u, h, hop, mode, wseed, K)
        figs.append(f)
        recs += r
    if halo:
        assert cfg.resblock == 2, "the f32 halo check exists for ResBlock2 voices only"
        check_halo(target, vname, path, case, recs, h, hop, wseed)
    U.require(names, set(STAGE[path]) | set(wanted), (vname, path, case))
    return figs, recs


# ---- the cases: one compared play each, then every check
def case_one(target, vname, eng, emu, case, u, asks, halo=False, wanted=(), mode="f32", K="gate"):
    got, h, names = compared(eng, lambda us: play_one(eng, us[0], asks), [u], emu)
    return got, names, check_case(target, vname, "W", case, got, h, eng.hop, names, wanted, halo, mode, K=K)


def case_batch(target, vname, eng, emu, case, utts, chunk, halo=False, wanted=(), mode="f32", K="gate"):
    got, h, names = compared(eng, lambda us: play_batch(eng, us, chunk), utts, emu)
    return got, names, check_case(target, vname, "V", case, got, h, eng.hop, names, wanted, halo, mode, K=K)


def case_pool(target, vname, eng, emu, case, three, newcomer, leaver, first, chunk, max_frames, halo=True, wanted=()):
    """One pool for all plays of the case (closing a pool drops its graphs)."""
    pool = eng.stream_pool(3, max_frames)
    try:
        got, h, names = compared(eng, lambda us: play_pool(eng, pool, us[:3], us[3], leaver, first, chunk), three + [newcomer], emu)
        assert h == pool.halo
    finally:
        pool.close()
    for i, u in enumerate(got):
        want = P.expected_sizes(u.F, first, chunk)
        sizes = [a.size // eng.hop for a, _ in u.chunks]
        assert u.left == (i == leaver) and (sizes == want[:len(sizes)] and 0 < len(sizes) < len(want) if u.left else sizes == want), (u.name, sizes, want)
    return got, names, check_case(target, vname, "P", case, got, h, eng.hop, names, wanted, halo)


def print_tables(target):
    print("\n| target | voice | path | case | mode | utterance | F | chunks | e_hip | e_ref | ratio | r_hip | r_ref | ratio | worst chunk / pooled e_ref | precondition |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for tg, v, path, case, mode, name, F, n, eh, er, rh, rr, worst, pre in ROWS:
        if tg == target:
            print(f"| {tg} | {v} | {path} | {case} | {mode} | {name} | {F} | {n} | {eh:.2e} | {er:.2e} | {eh / max(er, 1e-300):.2f} | {rh:.2e} | "
                  f"{rr:.2e} | {rh / max(rr, 1e-300):.2f} | {worst:.2f} | {pre:.1e} |")
    print("\n| target | voice | path | case | side | chunks | s(f32 of A) | s(f32 of B) | s(engine) |\n|---|---|---|---|---|---|---|---|---|")
    for tg, v, path, case, side, n, sa, sb, sh in HALO:
        if tg == target:
            print(f"| {tg} | {v} | {path} | {case} | {side} | {n} | {sa:+.4f} | {sb:.4f} | {sh:+.4f} |")
    print("\n| target | voice | path | case | kernels |\n|---|---|---|---|---|")
    for (tg, v, path, case), names in KERNELS.items():
        if tg == target:
            print(f"| {tg} | {v} | {path} | {case} | {' '.join(names)} |")
