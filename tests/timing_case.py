"""Timing plans (pe_timing: per-id rates, forced durations, a target frame count): what
tests/test_timing_emu.py and tests/test_gpu_timing.py share -- the inputs, the arithmetic restated in Python integers, a timed
oracle, and every check as a function of an engine.

The restatement starts from w, the f32 value the kernel itself publishes (w_out of pe_debug_timing, the debug tensor
"plan_w"): everything behind it is integer arithmetic and must be met exactly.

    no target   d_i = forced_i if forced_i >= 0 else clamp(ceil(w_i), 0, 1e6)
    target N    forced ids keep forced_i; the n free ids get 1 + a_i + extra_i with R = N - sum(forced) - n,
                q_i = max(1, trunc(min(w_i, 1e6) * 2^20)) if w_i > 0 else 1, Q = sum q_i, a_i = q_i R // Q, r_i = q_i R % Q,
                L = R - sum a_i; the L ids with the largest r_i, ties to the lower index, have extra_i = 1
    frames      max(sum d_i, 1), clamped to MAX_FRAMES + 1

The timed oracle is composed of public pieces of oracle/vits_oracle.py: text_encoder for m_p and logs_p, np.repeat by the
given integer durations, z_p = m + noise_z * exp(logs) * noise_scale, decode(..., dtype=float32). It is handed the engine's
own durations after those have been checked exactly against the restatement, so no ceil flip can make the two incomparable."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests", "emu")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
from oracle import vits_oracle as O                      # noqa: E402
from piper_amd import _lib as L, weights as W            # noqa: E402
from piper_amd.engine import Engine, EngineError, Timing  # noqa: E402
import stream_batch_case as K                            # noqa: E402

MAX_FRAMES = 60000
KERNEL_T = (1, 6, 255, 256, 257, 300, 4097, 8192)


# ---- the restatement
def restate(w, forced, target):
    """(durations, frames) of one utterance from the kernel's own w (float32), forced (-1 = free) and target (0 = none)."""
    w = np.asarray(w, np.float32)
    forced = np.asarray(forced, np.int64)
    T = w.size
    d = [0] * T
    free = [i for i in range(T) if forced[i] < 0]
    for i in range(T):
        if forced[i] >= 0:
            d[i] = int(forced[i])
        else:
            c = np.ceil(w[i])
            d[i] = int(min(max(c, np.float32(0)), np.float32(1.0e6)))
    if target > 0 and free:
        R = int(target) - sum(int(forced[i]) for i in range(T) if forced[i] >= 0) - len(free)
        assert R >= 0
        q = {}
        for i in free:
            if w[i] > 0:
                x = np.float32(min(w[i], np.float32(1.0e6))) * np.float32(1048576.0)      # exact: a power of two
                q[i] = max(1, int(x))                      # int() truncates
            else:
                q[i] = 1
        Q = sum(q.values())
        a = {i: q[i] * R // Q for i in free}
        r = {i: q[i] * R % Q for i in free}
        Lx = R - sum(a.values())
        assert 0 <= Lx < len(free)
        extra = set(sorted(free, key=lambda i: (-r[i], i))[:Lx])
        for i in free:
            d[i] = 1 + a[i] + (1 if i in extra else 0)
        assert sum(d) == target
    s = sum(d)
    return np.asarray(d, np.int64), (1 if s < 1 else (MAX_FRAMES + 1 if s > MAX_FRAMES else s))


def w_float32(logw, length_scale, rate):
    """w in np.float32 arithmetic, in the kernel's order."""
    return (np.exp(np.asarray(logw, np.float32)) * np.float32(length_scale)) * np.asarray(rate, np.float32)


def check_kernel_rows(eng, rows, scales, rate, forced, target, what):
    """pe_debug_timing on `rows` under the plan; durations and frames must equal the restatement from the kernel's own w."""
    B = len(rows)
    t = Timing(rate=rate, durations=forced, target_frames=target)
    dur, frames, w = eng.debug_timing(rows, scales, t)
    for b in range(B):
        f = np.full(len(rows[b]), -1, np.int64) if forced is None or forced[b] is None else np.asarray(forced[b], np.int64)
        N = 0 if target is None else int(target[b])
        want, fr = restate(w[b], f, N)
        assert np.array_equal(dur[b], want), (what, b, np.flatnonzero(dur[b] != want)[:8], dur[b][:8], want[:8])
        assert int(frames[b]) == fr, (what, b, int(frames[b]), fr)
        if N > 0 and fr <= MAX_FRAMES:
            assert int(frames[b]) == N and int(dur[b].sum()) == N, (what, b)
    return dur, frames, w


# ---- case 1: the kernel alone
def check_kernel_alone(eng):
    rng = np.random.default_rng(5)
    scales = np.array([[0.667, 1.0, 0.8], [0.5, 0.7, 0.8], [0.5, 1.3, 0.8], [0.667, 1.0, 0.8], [0.4, 0.9, 0.8]], np.float32)
    for T in KERNEL_T:
        # five utterances of T ids: plain, rates only, some ids forced, target only, target with forced ids and rates
        rows = [rng.normal(0.5, 0.8, T).astype(np.float32) for _ in range(5)]
        rate = [None, rng.uniform(0.5, 2.0, T).astype(np.float32), None, None, rng.uniform(0.5, 2.0, T).astype(np.float32)]
        f2 = np.where(rng.random(T) < 0.3, rng.integers(0, 6, T), -1).astype(np.int32)
        f4 = np.where(rng.random(T) < 0.3, rng.integers(0, 6, T), -1).astype(np.int32)
        if T > 1:
            f4[int(rng.integers(0, T))] = -1             # at least one free id under the target
        forced = [None, None, f2, None, f4]
        n4, s4 = int((f4 < 0).sum()), int(f4[f4 >= 0].sum())
        t3 = min(MAX_FRAMES, max(T, int(2.7 * T) + 3))
        t4 = min(MAX_FRAMES, s4 + n4 + int(1.9 * n4) + 1) if n4 else s4
        if n4 == 0 and s4 == 0:                          # (T == 1 with its id forced to 0 frames: not a valid plan)
            f4[0], t4 = 3, 3
        if not (f2 < 0).any() and f2.sum() == 0:
            f2[0] = 2
        target = [0, 0, 0, t3, t4]
        check_kernel_rows(eng, rows, scales, rate, forced, target, f"modes T={T}")
    # ties: all logw equal and R no multiple of n -- only the index rule decides who gets the extras
    for T, N in ((7, 7 + 12), (300, 300 + 457), (4097, 4097 + 5000)):
        rows = [np.full(T, 0.25, np.float32)]
        dur, _, _ = check_kernel_rows(eng, rows, (0.667, 1.0, 0.8), None, None, [N], f"ties T={T}")
        R = N - T
        assert R % T != 0
        want = np.full(T, 1 + R // T)
        want[:R % T] += 1
        assert np.array_equal(dur[0], want), ("ties", T)
    # w clamps at 1e6 (logw = +40), q = 1 (logw = -40), and the two mixed under one target
    big, small = np.full(9, 40.0, np.float32), np.full(9, -40.0, np.float32)
    mix = np.where(np.arange(300) % 3 == 0, 40.0, -40.0).astype(np.float32)
    dur, frames, w = check_kernel_rows(eng, [big, small, mix, big, small], (0.667, 1.0, 0.8), None, None, [0, 0, 0, 1000, 1000],
                                       "clamps")
    assert np.all(dur[0] == 1000000) and frames[0] == MAX_FRAMES + 1 and np.all(dur[1] == 1) and frames[1] == 9
    assert np.all(w[3] > 1.0e6) and np.all((w[4] > 0) & (w[4] < 1e-10))
    check_kernel_rows(eng, [mix], (0.667, 1.0, 0.8), None, None, [3000], "clamps mixed")
    # target == sum(forced) + n: every free id gets one frame
    T = 257
    f = np.where(np.arange(T) % 5 == 0, 4, -1).astype(np.int32)
    N = int(f[f >= 0].sum() + (f < 0).sum())
    dur, _, _ = check_kernel_rows(eng, [rng.normal(0.5, 0.8, T).astype(np.float32)], (0.667, 1.0, 0.8), None, [f], [N], "minimal target")
    assert np.all(dur[0][f < 0] == 1)
    # target == MAX_FRAMES
    for T in (300, 8192):
        check_kernel_rows(eng, [rng.normal(0.5, 0.8, T).astype(np.float32)], (0.667, 1.0, 0.8), None, None, [MAX_FRAMES], f"max target T={T}")
    # every id forced: with and without the matching target
    f = rng.integers(0, 7, 300).astype(np.int32)
    check_kernel_rows(eng, [rng.normal(0, 1, 300).astype(np.float32)] * 2, (0.667, 1.0, 0.8), None, [f, f], [0, int(f.sum())], "all forced")


def check_w_against_float32(eng):
    """|logw| <= 20: w_out within 1e-6 relative of np.float32 arithmetic -- 8 ulp of f32: two correctly rounded
    multiplications plus an expf of at most 2 ulp on either side."""
    rng = np.random.default_rng(6)
    T = 4097
    rows = [rng.uniform(-20, 20, T).astype(np.float32), np.linspace(-20, 20, T).astype(np.float32)]
    rate = [rng.uniform(0.25, 4.0, T).astype(np.float32), None]
    sc = np.array([[0.667, 0.83, 0.8], [0.667, 1.0, 0.8]], np.float32)
    _, _, w = eng.debug_timing(rows, sc, Timing(rate=rate))
    worst = 0.0
    for b in range(2):
        want = w_float32(rows[b], sc[b, 1], np.ones(T, np.float32) if rate[b] is None else rate[b])
        rel = np.abs(w[b].astype(np.float64) - want.astype(np.float64)) / want.astype(np.float64)
        worst = max(worst, float(rel.max()))
    print(f"w_out against np.float32: worst relative error {worst:.3e}")
    assert worst <= 1e-6, worst


# ---- the timed oracle
def timed_oracle(wt, cfg, ids, durations, noise_z, noise_scale, sid=None):
    """(float audio, int16) of one utterance whose id i lasts durations[i] frames."""
    d = np.asarray(durations, np.int64)
    with torch.no_grad():
        ids_t = torch.as_tensor(np.asarray(ids), dtype=torch.long).view(1, -1)
        _, m, logs, _ = O.text_encoder(wt, cfg, ids_t, torch.tensor([ids_t.shape[1]], dtype=torch.long))
    m, logs = m[0].numpy().astype(np.float32), logs[0].numpy().astype(np.float32)
    Fr = int(d.sum())
    assert Fr >= 1
    me, le = np.repeat(m, d, axis=1), np.repeat(logs, d, axis=1)
    z_p = me + np.asarray(noise_z, np.float32)[:, :Fr] * np.exp(le) * np.float32(noise_scale)
    audio = O.decode(wt, cfg, z_p.astype(np.float32), sid=sid, dtype=torch.float32)
    return audio, O.audio_float_to_int16(audio)


def assert_audio(got_a, got_p, ref_a, ref_p, gate, what):
    assert got_a.shape == ref_a.shape == got_p.shape, (what, got_a.shape, ref_a.shape)
    err = float(np.max(np.abs(got_a - ref_a)))
    rms = float(np.sqrt(np.mean(((got_p.astype(np.float64) - ref_p) / 32767.0) ** 2)))
    print(f"{what}: float max err {err:.3e} (gate {gate:g}), pcm rms {rms:.3e}")
    assert np.array_equal(O.audio_float_to_int16(got_a), got_p), what      # 0 LSB on the engine's own floats
    assert err < gate, (what, err)
    assert rms <= 1e-3, (what, rms)


class Voice:
    """A tiny voice with its inputs: the 6, 14 and 23 ids of stream_batch_case.inputs."""

    def __init__(self, preset, lib=None, device=0):
        self.ms = preset.endswith("-ms")
        self.cfg = W.preset(preset)
        self.w = W.synthetic_weights(self.cfg, 1234)
        self.wt = O.to_torch(self.w)
        self.eng = Engine(blob=W.pack_blob(self.cfg, self.w), lib=lib, device=device)
        self.ids, self.nw, self.nz = K.inputs(self.cfg)
        self.scales = K.SCALES_MS if self.ms else K.SCALES
        self.sids = list(K.SIDS) if self.ms else None

    def close(self):
        self.eng.close()

    def sub(self, idx):
        """ids, scales, sids, noise of the utterances idx (a list; repeats allowed)."""
        return ([self.ids[i] for i in idx], np.ascontiguousarray(self.scales[idx]), None if self.sids is None else [self.sids[i] for i in idx],
                np.ascontiguousarray(self.nw[idx]), np.ascontiguousarray(self.nz[idx]))


def split(flat, id_lists):
    offs = np.concatenate([[0], np.cumsum([len(s) for s in id_lists])])
    return [np.asarray(flat[offs[b]:offs[b + 1]]) for b in range(len(id_lists))]


# ---- case 2: a plan that says nothing
def check_silent_plan(v):
    eng = v.eng
    ids, sc, sids, nw, nz = v.sub([0, 1, 2])
    base = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz)
    base_d = eng.durations()
    plans = [Timing(rate=[np.ones(len(s), np.float32) for s in ids], durations=[np.full(len(s), -1) for s in ids], target_frames=[0, 0, 0]),
             Timing()]
    for k, t in enumerate(plans):
        r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=t)
        assert np.array_equal(eng.durations(), base_d), k
        assert np.array_equal(r.frames, base.frames), k
        for b in range(3):
            assert np.array_equal(r.audio[b], base.audio[b]) and np.array_equal(r.pcm[b], base.pcm[b]), (k, b)


# ---- case 3: round trip
def check_round_trip(v, gate):
    eng = v.eng
    ids, sc, sids, nw, nz = v.sub([0, 1, 2])
    base = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz)
    d = split(eng.durations(), ids)
    forced = Timing(durations=d)
    rng = np.random.default_rng(9)
    other_nw = rng.standard_normal(nw.shape).astype(np.float32)
    sc2 = sc.copy()
    sc2[:, 2] = [0.1, 1.7, 0.0]                          # another noise_w scale per utterance
    launches = []
    for nwx, scx in ((nw, sc), (other_nw, sc), (None, sc2), (other_nw, sc2)):
        r = eng.synthesize_batch(ids, scx, sids=sids, noise_w=nwx, noise_z=nz, timing=forced)
        launches.append(eng.run_launches)
        assert np.array_equal(r.frames, base.frames)
        assert all(np.array_equal(a, b) for a, b in zip(split(eng.durations(), ids), d))
        for b in range(3):
            assert np.array_equal(r.audio[b], base.audio[b]) and np.array_equal(r.pcm[b], base.pcm[b]), b
        with_msg = None
        for name in ("logw", "plan_w"):
            try:
                eng.debug_tensor(name, 0)
            except EngineError as e:
                with_msg = str(e)
                assert "not available" in with_msg and "forced" in with_msg, with_msg
            else:
                raise AssertionError(f"{name} of an all-forced call must not be available")
    # one id left free: the duration predictor runs again, which costs launches
    d1 = [x.copy() for x in d]
    d1[1][3] = -1
    eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=Timing(durations=d1))
    one_free = eng.run_launches
    assert eng.debug_tensor("plan_w", 1).shape == (1, len(ids[1]))
    assert all(n < one_free for n in launches), (launches, one_free)
    print(f"launches: all forced {launches[0]}, one id free {one_free}")
    if v.ms:
        # the same timing with other speakers: durations identical, audio that of the speaker's timed oracle
        other = [(s + 1) % v.cfg.n_speakers for s in sids]
        r = eng.synthesize_batch(ids, sc, sids=other, noise_w=nw, noise_z=nz, timing=forced)
        assert all(np.array_equal(a, b) for a, b in zip(split(eng.durations(), ids), d))
        for b in range(3):
            ra, rp = timed_oracle(v.wt, v.cfg, ids[b], d[b], nz[b], sc[b, 0], sid=other[b])
            assert_audio(r.audio[b], r.pcm[b], ra, rp, gate, f"round trip, speaker {other[b]} on utterance {b}")
            assert not np.array_equal(r.pcm[b], base.pcm[b])


# ---- case 4: a mixed timed batch
def mixed_plan(v):
    """Four utterances (6, 14, 23 and the 14 ids again), one plan each: rates from 0.5 to 2; two forced ids, one of them 0
    frames; a target 30 % below the natural length; a target 30 % above it. Returns (idx, plan pieces, natural frames)."""
    idx = [0, 1, 2, 1]
    ids, sc, sids, nw, nz = v.sub(idx)
    nat = v.eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz).frames
    rate = [np.linspace(0.5, 2.0, len(ids[0])).astype(np.float32), None, None, None]
    f1 = np.full(len(ids[1]), -1, np.int32)
    f1[2], f1[9] = 0, 7
    forced = [None, f1, None, None]
    target = [0, 0, int(round(0.7 * int(nat[2]))), int(round(1.3 * int(nat[3])))]
    assert target[2] >= len(ids[2]) and target[2] < nat[2] < MAX_FRAMES and target[3] > nat[3], (target, nat)
    return idx, rate, forced, target, nat


def check_mixed(v, gate, oracle=True):
    eng = v.eng
    idx, rate, forced, target, nat = mixed_plan(v)
    ids, sc, sids, nw, nz = v.sub(idx)
    t = Timing(rate=rate, durations=forced, target_frames=target)
    r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=t)
    d = split(eng.durations(), ids)
    for b in range(len(ids)):
        w = eng.debug_tensor("plan_w", b)[0]
        f = np.full(len(ids[b]), -1) if forced[b] is None else forced[b]
        want, fr = restate(w, f, target[b])
        assert np.array_equal(d[b], want), (b, d[b], want)
        assert int(r.frames[b]) == fr and (target[b] == 0 or fr == target[b]), (b, r.frames[b], fr)
        assert r.audio[b].size == fr * eng.hop
        logw = eng.debug_tensor("logw", b)[0]
        want_w = w_float32(logw, sc[b, 1], np.ones(len(ids[b]), np.float32) if rate[b] is None else rate[b])
        assert np.all(np.abs(w - want_w) <= 1e-6 * want_w), b
        if oracle:
            ra, rp = timed_oracle(v.wt, v.cfg, ids[b], d[b], nz[b], sc[b, 0], sid=None if sids is None else sids[b])
            assert_audio(r.audio[b], r.pcm[b], ra, rp, gate, f"mixed batch, utterance {b}")
    assert d[1][2] == 0 and d[1][9] == 7
    assert int(r.frames[0]) != int(nat[0])               # (the rates did move something)
    return r, d


# ---- case 5: batch independence
def check_batch_independence(v):
    eng = v.eng
    idx, rate, forced, target, _ = mixed_plan(v)
    ids, sc, sids, nw, nz = v.sub(idx)
    r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=Timing(rate=rate, durations=forced, target_frames=target))
    d = split(eng.durations(), ids)
    for b in range(len(ids)):
        one = eng.synthesize_batch([ids[b]], sc[b:b + 1], sids=None if sids is None else [sids[b]], noise_w=nw[b:b + 1], noise_z=nz[b:b + 1],
                                   timing=Timing(rate=[rate[b]], durations=[forced[b]], target_frames=[target[b]]))
        assert np.array_equal(eng.durations(), d[b]), b
        assert one.audio[0].shape == r.audio[b].shape and np.max(np.abs(one.audio[0] - r.audio[b])) < 1e-5, b


# ---- case 6: targets are exact everywhere
def drain_batch(eng, ids, sc, sids, nw, nz, timing, chunk=K.CHUNK):
    per = [[] for _ in ids]
    for item in eng.stream_batch(ids, sc, sids=sids, chunk_frames=chunk, noise_w=nw, noise_z=nz, timing=timing):
        for b, (a, p) in enumerate(item):
            if p.size:
                per[b].append((a, p))
    return per


def check_targets_exact(v):
    import resample_case as RS
    eng = v.eng
    ids, sc, sids, nw, nz = v.sub([0, 1, 2])
    target = [17, 40, 29]
    t = Timing(target_frames=target)
    r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=t)
    assert list(r.frames) == target and [a.size for a in r.audio] == [f * eng.hop for f in target]
    per = drain_batch(eng, ids, sc, sids, nw, nz, t)
    assert list(eng.stream_frames) == target
    assert [sum(p.size for _, p in c) for c in per] == [f * eng.hop for f in target]
    with eng.stream_pool(3, 40) as pool:
        slots = pool.join(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=t)      # 40 == max_frames: accepted
        assert slots == [0, 1, 2] and list(pool.frames) == target
        pool.next(K.CHUNK)
        for s in (0, 2):
            pool.leave(s)
        state = (pool.frames, pool.frames_done, pool.free_slots)
        try:
            pool.join([ids[0]], sc[:1], sids=None if sids is None else sids[:1], noise_w=nw[:1], noise_z=nz[:1],
                      timing=Timing(target_frames=[41]))
        except EngineError as e:
            assert "max_frames" in str(e) and "41" in str(e), str(e)
        else:
            raise AssertionError("a target of max_frames + 1 must be refused")
        assert np.array_equal(pool.frames, state[0]) and np.array_equal(pool.frames_done, state[1]) and pool.free_slots == state[2]
        got = 0
        while True:
            out = pool.next(K.CHUNK)
            if not out:
                break
            assert list(out) == [1]
            got += out[1][1].size
        assert got + K.CHUNK * eng.hop == 40 * eng.hop
    # at 8000 Hz the delivered sample count is that of any utterance of the same frame count
    nat = eng.native_rate
    eng.set_output_rate(8000)
    try:
        r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=t)
        assert list(r.frames) == target
        assert [p.size for p in r.pcm] == [RS.n_out(f * eng.hop, nat, 8000) for f in target]
        un = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz)
        rt = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=Timing(target_frames=[int(f) for f in un.frames]))
        assert [p.size for p in rt.pcm] == [p.size for p in un.pcm]
    finally:
        eng.set_output_rate(None)


# ---- case 7: streams
def check_streams(v):
    eng = v.eng
    idx, rate, forced, target, _ = mixed_plan(v)
    ids, sc, sids, nw, nz = v.sub(idx)
    t = Timing(rate=rate, durations=forced, target_frames=target)
    full = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=t)
    per = drain_batch(eng, ids, sc, sids, nw, nz, t)
    assert np.array_equal(eng.stream_frames, full.frames)
    for b in range(len(ids)):
        assert [p.size for _, p in per[b]][:-1] == [K.CHUNK * eng.hop] * (len(per[b]) - 1)
        cat = np.concatenate([a for a, _ in per[b]])
        assert cat.shape == full.audio[b].shape and np.max(np.abs(cat - full.audio[b])) < 1e-5, b
    # a timed newcomer (the 23 ids under the 30 % shorter target) joins two untimed residents
    res = v.sub([0, 1])
    new = v.sub([2])
    tn = Timing(target_frames=[target[2]])

    def play(with_newcomer):
        chunks = {0: [], 1: [], 2: []}
        with eng.stream_pool(3, 64) as pool:
            assert pool.join(res[0], res[1], sids=res[2], noise_w=res[3], noise_z=res[4]) == [0, 1]
            k = 0
            while True:
                out = pool.next(K.CHUNK)
                if not out:
                    break
                for s, c in out.items():
                    chunks[s].append(c)
                k += 1
                if k == 1 and with_newcomer:
                    assert pool.join(new[0], new[1], sids=new[2], noise_w=new[3], noise_z=new[4], timing=tn) == [2]
                    assert pool.frames[2] == target[2]
        return chunks

    alone, joined = play(False), play(True)
    for s in (0, 1):
        assert len(alone[s]) == len(joined[s]) > 0
        for (a, p), (a1, p1) in zip(alone[s], joined[s]):
            assert np.array_equal(a, a1) and np.array_equal(p, p1), s
    own = drain_batch(eng, new[0], new[1], new[2], new[3], new[4], tn)[0]
    assert len(own) == len(joined[2]) == -(-target[2] // K.CHUNK)
    for (a, p), (a1, p1) in zip(own, joined[2]):
        assert a.shape == a1.shape and np.max(np.abs(a - a1)) < 1e-5
        assert np.array_equal(O.audio_float_to_int16(a1), p1)


# ---- case 8: errors
def check_errors(v):
    """Every rule of the plan refused with its message between two chunks of a live batch stream, which completes unchanged."""
    eng, lib = v.eng, v.eng._lib
    ids, sc, sids, nw, nz = v.sub([0, 1, 2])
    want = drain_batch(eng, ids, sc, sids, nw, nz, None)
    flat = np.ascontiguousarray(np.concatenate(ids), np.int64)
    off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int64)
    n = flat.size
    p64, pf, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    sd = None if sids is None else np.ascontiguousarray(sids, np.int64)
    frames, halo, res = (C.c_int32 * 3)(), C.c_int32(), L.PeResult()

    def plan(rate=None, forced=None, target=None):
        keep = []
        t = L.PeTiming()
        if rate is not None:
            keep.append(np.ascontiguousarray(rate, np.float32))
            t.rate = keep[-1].ctypes.data_as(pf)
        if forced is not None:
            keep.append(np.ascontiguousarray(forced, np.int32))
            t.forced = keep[-1].ctypes.data_as(p32)
        if target is not None:
            keep.append(np.ascontiguousarray(target, np.int32))
            t.target_frames = keep[-1].ctypes.data_as(p32)
        return t, keep

    def refused(t, text, entry=0):
        a = (eng._h, flat.ctypes.data_as(p64), off.ctypes.data_as(p64), 3, sc.ctypes.data_as(pf), None if sd is None else sd.ctypes.data_as(p64), None)
        if entry == 0:
            rc = lib.pe_stream_begin_batch_timed(*a, frames, C.byref(halo), C.byref(t[0]))
        elif entry == 1:
            rc = lib.pe_upload_timed(*a, C.byref(t[0]))
        else:
            rc = lib.pe_synthesize_batch_timed(*a, C.byref(res), C.byref(t[0]))
        msg = lib.pe_last_error().decode()
        assert rc != 0 and all(s in msg for s in text), (msg, text)

    ones, free = np.ones(n, np.float32), np.full(n, -1, np.int32)
    r_nan, r_zero, r_inf = ones.copy(), ones.copy(), ones.copy()
    r_nan[off[1] + 4], r_zero[2], r_inf[off[2]] = np.nan, 0.0, np.inf
    f_m2, f_big = free.copy(), free.copy()
    f_m2[off[2] + 7], f_big[1] = -2, MAX_FRAMES + 1
    f_two = free.copy()
    f_two[off[1]:off[1] + 2] = 10                        # utterance 1: 20 forced frames + 12 free ids
    all3 = np.full(n, 3, np.int32)
    zero1 = all3.copy()
    zero1[off[1]:off[2]] = 0
    cases = [
        lambda: refused(plan(rate=r_nan), ("utterance 1", "id 4", "rate must be finite and > 0"), 0),
        lambda: refused(plan(rate=r_zero), ("utterance 0", "id 2", "rate must be finite and > 0"), 1),
        lambda: refused(plan(rate=r_inf), ("utterance 2", "id 0", "rate must be finite and > 0"), 2),
        lambda: refused(plan(forced=f_m2), ("utterance 2", "id 7", "forced duration -2 outside [-1, 60000]"), 0),
        lambda: refused(plan(forced=f_big), ("utterance 0", "id 1", "forced duration 60001 outside"), 1),
        lambda: refused(plan(target=[0, -1, 0]), ("utterance 1", "target_frames -1 outside [0, 60000]"), 2),
        lambda: refused(plan(target=[0, 0, MAX_FRAMES + 1]), ("utterance 2", "target_frames 60001 outside"), 0),
        lambda: refused(plan(forced=f_two, target=[0, 31, 0]), ("utterance 1", "target_frames 31 is below", "sum 20", "12 free ids"), 0),
        lambda: refused(plan(target=[5, 0, 0]), ("utterance 0", "target_frames 5 is below", "6 free ids"), 1),
        lambda: refused(plan(forced=all3, target=[18, 41, 69]), ("utterance 1", "every id is forced", "sum 42 differs from target_frames 41"), 2),
        lambda: refused(plan(forced=zero1), ("utterance 1", "every id is forced", "sum 0 is outside [1, 60000]"), 0),
    ]
    per = [[] for _ in ids]
    k = -1
    for k, item in enumerate(eng.stream_batch(ids, sc, sids=sids, chunk_frames=2, noise_w=nw, noise_z=nz)):
        for b, (a, p) in enumerate(item):
            if p.size:
                per[b].append((a, p))
        if k < len(cases):
            cases[k]()
    assert k + 1 >= len(cases), (k, len(cases))
    for b in range(3):
        assert np.array_equal(np.concatenate([a for a, _ in per[b]]), np.concatenate([a for a, _ in want[b]])), b
    # accepted at the edge: target == sum(forced) + n, and an all-forced plan that matches its target
    r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=Timing(durations=split(f_two, ids), target_frames=[0, 32, 0]))
    assert r.frames[1] == 32
    r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz, timing=Timing(durations=split(all3, ids), target_frames=[18, 42, 69]))
    assert list(r.frames) == [18, 42, 69]
    # the pool: a refused timed join leaves it as it was
    with eng.stream_pool(2, 64) as pool:
        try:
            pool.join(ids[:1], sc[:1], sids=None if sids is None else sids[:1], noise_w=nw[:1], noise_z=nz[:1], timing=Timing(target_frames=[3]))
        except EngineError as e:
            assert "target_frames 3 is below" in str(e)
        else:
            raise AssertionError("refusal expected")
        assert pool.free_slots == [0, 1]


# ---- case 9: the untimed path is untouched
def check_untimed_untouched(v):
    eng = v.eng
    ids, sc, sids, nw, nz = v.sub([0, 1, 2])
    one, sc1, sid1 = [ids[2]], tuple(float(x) for x in sc[2]), None if sids is None else [sids[2]]
    # with injected noise: the same PCM and the same launches before and after a burst of timed calls
    a = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz)
    la = eng.run_launches
    # with the engine's own prior noise (the duration noise stays injected, so the frame count is the same every time): two
    # calls, the second of which is sized from the first's frames per id where the engine speculates
    nw1 = nw[2:3]
    eng.synthesize_batch(one, sc1, sids=sid1, noise_w=nw1)
    r0 = eng.synthesize_batch(one, sc1, sids=sid1, noise_w=nw1)
    lu, stats, caps = eng.run_launches, eng.speculation_stats, eng.graph_stats[1]
    nat = int(r0.frames[0])
    for k in range(2):                                   # frames per id far below and above the voice's own
        t = Timing(target_frames=[len(one[0]) + (2 * nat if k % 2 else 0)])
        r = eng.synthesize_batch(one, sc1, sids=sid1, noise_w=nw1, timing=t)
        assert r.frames[0] == t.target_frames[0]
    eng.upload(one, sc1, sids=sid1, noise_w=nw1, timing=Timing(rate=[np.full(len(one[0]), 2.0, np.float32)]))
    eng.run()
    eng.run()                                            # (a repeated run keeps the plan)
    assert eng.fetch().frames[0] > 1.5 * nat
    assert eng.speculation_stats == stats                # timed calls: no speculative run, no miss
    caps_timed = eng.graph_stats[1]
    r1 = eng.synthesize_batch(one, sc1, sids=sid1, noise_w=nw1)
    assert r1.frames[0] == nat and eng.run_launches == lu
    assert eng.graph_stats[1] == caps_timed              # sized as before the burst: the graph it replays exists already
    s1 = eng.speculation_stats
    assert s1[1] == stats[1] and s1[0] - stats[0] == (1 if stats[0] > 0 else 0), (stats, s1)
    b = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, noise_z=nz)
    assert eng.run_launches == la
    for x, y in zip(a.pcm, b.pcm):
        assert np.array_equal(x, y)
    return caps


def mixed_digest(v):
    """Durations and a digest of the int16 output of case 4 (the wave-order child process)."""
    r, d = check_mixed(v, 1e-4, oracle=False)
    h = hashlib.sha256()
    for p in r.pcm:
        h.update(np.ascontiguousarray(p).tobytes())
    return {"durations": [[int(x) for x in row] for row in d], "frames": [int(f) for f in r.frames], "pcm_sha256": h.hexdigest()}


# ---- PiperVoice and the JSONL driver
def check_voice_and_driver(lib, tmp_path):
    """durations= / rate= / target_seconds= of PiperVoice and the per-line keys of piper_amd.infer on the golden tiny voice:
    frames = round(seconds * native rate / hop), the delivered length follows from the output rate."""
    import io
    import json
    import wave
    import resample_case as RS
    from piper_amd import infer
    from piper_amd.config import PiperConfig
    from piper_amd.voice import PiperVoice
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    conf = PiperConfig.from_dict(json.load(open(model + ".json", encoding="utf-8")))
    voice = PiperVoice(session=Engine(onnx_path=model, lib=lib), config=conf)
    eng, sr = voice.session, int(conf.sample_rate)
    hop = eng.hop
    ids = [int(x) for x in W.synthetic_phoneme_ids(9, 3, id_max=39)]
    plain = voice.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0)
    d = eng.durations()
    assert len(plain) == 2 * hop * int(d.sum())
    again = voice.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0, durations=[int(x) for x in d])
    assert again == plain
    frames = int(round(0.5 * sr / hop))
    assert voice.target_frames(0.5) == frames and voice.target_frames(None) == 0
    fit = voice.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0, target_seconds=0.5)
    assert len(fit) == 2 * hop * frames
    slow = voice.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0, rate=[3.0] * len(ids))
    assert len(slow) > 2 * len(plain)
    two = voice.synthesize_ids_batch_to_raw([ids, ids[:5]], noise_scale=0.0, noise_w=0.0, durations=[None, [2, 0, 3, -1, 1]],
                                            target_seconds=[0.5, None])
    assert len(two[0]) == 2 * hop * frames and two[0] == fit
    assert eng.durations()[len(ids):][[0, 1, 2, 4]].tolist() == [2, 0, 3, 1]
    eng.set_output_rate(8000, native=sr)
    low = PiperVoice(session=eng, config=conf, output_sample_rate=8000).synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0, target_seconds=0.5)
    assert len(low) == 2 * RS.n_out(frames * hop, sr, 8000)
    eng.close()
    # the driver: a group with a timed line is one timed call, a group without is the call it was
    lines = [json.dumps({"phoneme_ids": ids, "target_seconds": 0.5}), json.dumps({"phoneme_ids": ids}),
             json.dumps({"phoneme_ids": ids[:5], "durations": [2, 0, 3, 4, 1]}),
             json.dumps({"phoneme_ids": ids, "rate": [3.0] * len(ids), "noise_w": 0.0})]
    out = tmp_path / "wavs"
    assert infer.main(["--model", model, "--output-dir", str(out), "--sample-rate", str(sr), "--batch", "2", "--seed", "3"],
                      stdin=io.StringIO("\n".join(lines)), lib=lib) == 0
    n = {}
    for k in range(4):
        with wave.open(str(out / f"{k}.wav"), "rb") as wv:
            assert wv.getframerate() == sr
            n[k] = wv.getnframes()
    assert n[0] == frames * hop and n[2] == 10 * hop and n[1] > 0 and n[1] % hop == 0 and n[3] > 2 * len(plain) // 2


# ---- the 192-channel small-call path
def check_192_channels(lib):
    """Round trip and a target on a voice with the 192 hidden channels of the medium / high qualities, tiny everywhere else:
    stage A takes the small-call forms there (the stacked enc_p.proj + dp.pre launch among them), and an all-forced call
    must still give the untimed call's audio bit for bit."""
    cfg = W.preset("tiny", hidden=192, inter=192, filter=96, n_layers=2)
    w = W.synthetic_weights(cfg, 1234)
    lens = [9, 31]
    ids = [W.synthetic_phoneme_ids(T, i, id_max=cfg.n_vocab - 1) for i, T in enumerate(lens)]
    rng = np.random.default_rng(5)
    nw = rng.standard_normal((2, 2, max(lens))).astype(np.float32)
    nz = rng.standard_normal((2, cfg.inter, 24 * max(lens) + 64)).astype(np.float32)
    sc = (0.5, 1.0, 0.8)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=lib)
    base = eng.synthesize_batch(ids, sc, noise_w=nw, noise_z=nz)
    d = split(eng.durations(), ids)
    r = eng.synthesize_batch(ids, sc, noise_z=nz, timing=Timing(durations=d))
    for b in range(2):
        assert np.array_equal(r.audio[b], base.audio[b]) and np.array_equal(r.pcm[b], base.pcm[b]), b
    target = [int(base.frames[0]) + 5, max(lens[1], int(0.8 * int(base.frames[1])))]
    r = eng.synthesize_batch(ids, sc, noise_w=nw, noise_z=nz, timing=Timing(target_frames=target))
    dt = split(eng.durations(), ids)
    for b in range(2):
        want, fr = restate(eng.debug_tensor("plan_w", b)[0], np.full(lens[b], -1), target[b])
        assert np.array_equal(dt[b], want) and int(r.frames[b]) == fr == target[b], b
    eng.close()
