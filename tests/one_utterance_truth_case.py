"""The one-utterance path stage by stage against f64 truths: what tests/test_gpu_one_utterance_truth.py (an MI355X) and
tests/test_one_utterance_truth_emu.py (the kernel emulator) share -- the cases, one run routine, and every check as a function.

Every stage is compared FROM THE ENGINE'S OWN INPUT to that stage (oracle.stage_truths): E ids -> x_enc, m_p, logs_p;
D the engine's x_enc and duration noise -> logw and w = exp(logw) * length_scale; R the engine's stats, integer durations
and prior noise -> z_p; F the engine's z_p -> z; G the engine's z -> audio. For a stage tensor with f64 truth t

    e_hip = max |engine - t|     e_ref = max |torch f32 - t|     r_hip, r_ref = the rms of the same differences
    fl    = 2^-23 * max |t|      (one f32 ulp of the peak)

    E, D (logw), F, G    e_hip <= K e_ref + fl   and   r_hip <= K r_ref          K per stage: GATES below
    durations            equal to ceil(w of the f64 stage D) for EVERY id; first the truth itself is asserted to stay
                         2e-5 * max(1, w) away from every integer (the project's figure for where a ceil may flip)
    R                    frames = max(sum d, 1); |z_p - (m + n)| <= 8 * 2^-24 * (|m| + |n|) elementwise, m and
                         n = noise * exp(logs) * noise_scale gathered by generate_path's own assignment of ids to frames:
                         one expf of at most 2 ulp plus three roundings, with a factor 2 to spare
    kernels              every case names, from the level-2 profile, the kernels it is there for

K = 8 is the project's gate for "two f32 summation orders" (tests/test_gpu_matrix_truth.py). profiles/one_utterance_truth.md
holds the measured ratios per stage and route, and the reason for every K that is not 8.

The compared call. On the device a repeated one-utterance call is ONE graph (text encoder to int16, regulate_kernel
computing the durations itself), which runs only with the engine's own prior noise and without the profile. So `run`
calls twice with injected duration noise (the seeds keep the oracle's own durations >= 1e-4 from an integer) and the
engine's prior noise -- the first time with ids and noise reversed, so that no buffer of the first call can pass for the
second's -- checks from speculation_stats that the second call was that graph, takes every tensor (the noise
included: debug_tensor "noise_z") from it, and then repeats the call under the level-2 profile with that noise injected:
the kernel names are the repeat's, whose durations and z_p must equal the compared call's bit for bit. The emulator has
no graphs: one profiled call with injected noise."""
import contextlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import vits_oracle as O                      # noqa: E402
from piper_amd import _lib as L, weights as W            # noqa: E402
from piper_amd.engine import Engine                      # noqa: E402

SCALES = (0.667, 1.0, 0.8)
# {noise_scale, length_scale, noise_w} per utterance of a batched call that mixes them (the first MIXED_SCALES[:B]): f32, as
# the engine takes them, so that a truth is computed at the very values
MIXED_SCALES = np.array([(0.667, 1.0, 0.8), (0.5, 1.3, 0.6), (0.8, 0.85, 1.0), (0.3, 1.15, 0.4), (0.9, 0.75, 0.9), (1.0, 1.0, 0.2),
                         (0.1, 1.4, 0.7), (0.667, 0.9, 0.5)], np.float32)
PRODUCT_GATE = 2e-4          # max |d audio| of the f32 path's own parity gate
CEIL_FLIP = 2e-5             # relative distance from an integer below which a ceil may flip in another summation order
STAGES = ("x_enc", "m_p", "logs_p", "logw", "z", "audio")
SM = {"bf16x3": 0, "f16x3": 1, "bf16x6": 2}           # PIPER_HIP_MATRIX -> the kernels' split mode template argument
WIDE = {"tiny192": dict(hidden=192, inter=192, filter=96, n_layers=2)}      # tiny with the 192 channels of medium / high

# K per stage tensor (max and rms gate alike), from the measured worst ratios in profiles/one_utterance_truth.md: 8 wherever
# the worst ratio is at most 4.
GATES = {"gpu": {s: 8 for s in STAGES}, "emu": {s: 8 for s in STAGES},
         # the batched path (tests/test_gpu_batched_truth.py, tests/test_batched_truth_emu.py; profiles/batched_truth.md)
         "gpu-batched": {s: 8 for s in STAGES}, "emu-batched": {s: 8 for s in STAGES}}
ORACLE_MARGIN = 1e-4         # relative distance from an integer that the chosen seeds keep with the oracle alone

ROWS = []        # (target, voice, lens, route, mode, utterance, stage, e_hip, e_ref, r_hip, r_ref): the table of the profile file
_VOICES = {}
_ENGINES = {}
_TRUTHS = {}


def truth_gates(err, mode, family):
    """The gates of tests/test_gpu_matrix_truth.py, from the operand bits: err = {setting: max |d audio| against f64},
    'torch' = the oracle's own f32 run, fl = 2^-23 * peak of the truth. One difference: the emulator rounds the f32
    accumulator after EVERY product of an MFMA (tests/emu/hip_emu.h), so bf16x6 takes six accumulator roundings per k
    element where the f32 kernel takes one: sqrt(6 + 1) ~ 2.65 times the f32 kernel's rounding error with the dropped
    2^-24 products, gate 3 here (2 on the hardware, whose bf16x6 lands below its f32 kernels: profiles/matrix_truth.md)."""
    fl = err["fl"]
    if mode == "f32":
        return err["f32"] <= 8 * err["torch"] + fl            # two f32 summation orders
    if mode == "bf16x6":
        return err[mode] <= 3 * err["f32"] + fl               # exact operands, dropped products at 2^-24, 6 roundings
    if mode == "f16x3":
        return err[mode] <= 4 * err["f32"] + fl if family != "rescaled" else err[mode] < PRODUCT_GATE   # 22 of 24 bits
    return err[mode] <= 2 ** 8 * err["f32"] and err[mode] < PRODUCT_GATE      # bf16x3: 16 of 24 bits


# ---- voices, inputs, engines
def voice(name, wseed=1234):
    """(cfg, weights) of a preset or of WIDE's variants; one dict object per voice, so oracle.content_key hashes it once."""
    if (name, wseed) not in _VOICES:
        cfg = W.preset("tiny", **WIDE[name]) if name in WIDE else W.preset(name)
        _VOICES[name, wseed] = (cfg, W.synthetic_weights(cfg, wseed))
    return _VOICES[name, wseed]


def one_inputs(cfg, T, index, seed):
    """One utterance as tests/test_gpu_kernel_entry.py draws it: ids and the duration noise [1][2][T]."""
    ids = W.synthetic_phoneme_ids(T, index, id_max=min(cfg.n_vocab - 1, 129))
    nw = np.random.default_rng(seed).standard_normal((2, T)).astype(np.float32)
    return [ids], nw[None]


def batch_inputs(cfg, lens, seed):
    """Utterance i = synthetic_phoneme_ids(lens[i], i); one draw [B][2][max T], then [B][C][32 max T + 64]."""
    ids = [W.synthetic_phoneme_ids(T, i, id_max=min(cfg.n_vocab - 1, 129)) for i, T in enumerate(lens)]
    rng = np.random.default_rng(seed)
    nw = rng.standard_normal((len(lens), 2, max(lens))).astype(np.float32)
    nz = rng.standard_normal((len(lens), cfg.inter, 32 * max(lens) + 64)).astype(np.float32)
    return ids, nw, nz


@contextlib.contextmanager
def policy_env(lib, env):
    """The process environment with every policy knob unset except `env` (knobs are read when an engine is created)."""
    knobs = [x["env"] for x in json.loads(lib.pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]
    saved = {k: os.environ.pop(k) for k in knobs if k in os.environ}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def engine_for(name, env=None, lib=None, wseed=1234, fresh=False):
    """One engine per (voice, environment), kept for the module: PIPER_HIP_DEBUG_KEEP=1 plus `env`. `fresh`: a new engine that
    the caller closes (its run counter, and with it the engine's own prior noise, starts where every fresh engine's does)."""
    env = dict(env or {})
    key = (name, wseed, tuple(sorted(env.items())), id(lib))
    if fresh or key not in _ENGINES:
        cfg, w = voice(name, wseed)
        the_lib = lib if lib is not None else L.get_lib()
        with policy_env(the_lib, dict(env, PIPER_HIP_DEBUG_KEEP=1)):
            eng = Engine(blob=W.pack_blob(cfg, w), lib=lib) if lib is not None else Engine(blob=W.pack_blob(cfg, w), device=0)
        if fresh:
            return eng
        _ENGINES[key] = eng
    return _ENGINES[key]


def close_engines():
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()
    _TRUTHS.clear()


# ---- one compared call
def _tensors(eng, r, ids):
    durs = eng.durations()
    off = np.concatenate([[0], np.cumsum([len(s) for s in ids])])
    out = []
    for b in range(len(ids)):
        out.append({"x_enc": eng.debug_tensor("x_enc", b), "stats": eng.debug_tensor("stats", b),
                    "logw": eng.debug_tensor("logw", b)[0], "durations": durs[off[b]:off[b + 1]].astype(np.int64),
                    "z_p": eng.debug_tensor("z_p", b), "z": eng.debug_tensor("z", b), "noise_w": eng.debug_tensor("noise_w", b),
                    "noise_z": eng.debug_tensor("noise_z", b), "audio": r.audio[b].copy(), "frames": int(r.frames[b])})
    return out


def _profiled(eng, ids, scales, sids, nw, nz):
    eng.profile_enable(2)
    eng.profile_reset()
    try:
        r = eng.synthesize_batch(ids, scales, sids=sids, noise_w=nw, noise_z=nz)
        names = {row["name"]: int(row["launches"]) for row in eng.profile()[5:] if row["launches"]}
    finally:
        eng.profile_enable(0)
    return r, names


def run(eng, ids, scales, sids, nw, nz=None, graph="spec"):
    """The compared call (module docstring): (per-utterance tensors, {kernel name: launches}). nz given: one profiled call with injected
    prior noise (the emulator). Otherwise graph = "spec" (the second call must be the whole-utterance graph), "two" (graphs,
    but PIPER_HIP_SPEC=0: none may be speculative) or "none" (PIPER_HIP_NO_GRAPH=1: nothing captured)."""
    if nz is not None:
        r, names = _profiled(eng, ids, scales, sids, nw, nz)
        return _tensors(eng, r, ids), names
    # the first call of a bucket (two graphs and a read-back) runs the SAME LENGTHS with every utterance's ids and duration noise
    # reversed: about the same frames per id for the speculation, but other values in every buffer debug_tensor reads, so a
    # buffer the compared call left stale could not pass for fresh (asserted below on the front half, whose values the profiled
    # repeat does not pin)
    other = [np.ascontiguousarray(np.asarray(s)[::-1]) for s in ids]
    onw = np.zeros_like(nw)
    top = 1 + max(int(np.max(s)) for s in ids)
    for b, s in enumerate(ids):
        onw[b, :, :len(s)] = nw[b, :, :len(s)][:, ::-1]
        if np.array_equal(other[b], s):          # a palindrome (one id of a batched call): the next id and the negated noise instead
            other[b], onw[b] = (np.asarray(s) + 1) % top, -nw[b]
    first = _tensors(eng, eng.synthesize_batch(other, scales, sids=sids, noise_w=onw), other)
    s0, g0 = eng.speculation_stats, eng.graph_stats
    r = eng.synthesize_batch(ids, scales, sids=sids, noise_w=nw)
    s1, g1 = eng.speculation_stats, eng.graph_stats
    if graph == "spec":
        assert s1[0] == s0[0] + 1 and s1[1] == s0[1], ("the compared call was not the one whole-utterance graph", s0, s1)
    else:
        assert s1 == s0, (graph, s0, s1)
        assert (g1[0] == 0) == (graph == "none"), (graph, g1)
    got = _tensors(eng, r, ids)
    for b, g in enumerate(got):
        for k in ("x_enc", "stats", "logw", "noise_w"):
            assert g[k].shape == first[b][k].shape and not np.array_equal(g[k], first[b][k]), (b, k, "the first call's values")
    C = got[0]["z_p"].shape[0]
    znz = np.zeros((len(ids), C, max(g["frames"] for g in got)), np.float32)
    for b, g in enumerate(got):
        assert g["noise_z"].shape == g["z_p"].shape == (C, g["frames"]) and np.any(g["noise_z"])
        znz[b, :, :g["frames"]] = g["noise_z"]
    rp, names = _profiled(eng, ids, scales, sids, nw, znz)
    rep = _tensors(eng, rp, ids)
    for b, g in enumerate(got):          # the names are the repeat's: it must be the same call
        assert np.array_equal(rep[b]["durations"], g["durations"]) and np.array_equal(rep[b]["z_p"], g["z_p"]), b
        assert np.array_equal(rep[b]["noise_z"], g["noise_z"]) and rep[b]["audio"].shape == g["audio"].shape, b
    return got, names


# ---- truths and figures
def _truth(w, cfg, stage, dtype, ids, scales, nw, nz, given, sid):
    """oracle.stage_truths of one stage, kept by the content of everything the stage reads: routes that leave a stage's input
    unchanged (most knobs touch one stage) share its truths, and nobody changes a kept array."""
    reads = {"E": (), "D": ("x_enc", nw), "R": ("stats", "durations", nz), "F": ("z_p",), "G": ("z",)}[stage]
    reads = [given[x] if isinstance(x, str) else x for x in reads]
    key = O.content_key(w, stage, str(dtype), np.asarray(ids), np.asarray(scales, np.float64), -1 if sid is None else int(sid), *reads)
    if key not in _TRUTHS:
        _TRUTHS[key] = O.stage_truths(w, cfg, ids, scales, nw, nz, given, sid=sid, dtype=dtype, stages=stage)
    return _TRUTHS[key]


def figures(hip, t64, t32):
    assert hip.shape == t64.shape == t32.shape, (hip.shape, t64.shape, t32.shape)
    dh, dr = hip.astype(np.float64) - t64, t32.astype(np.float64) - t64
    return {"e_hip": float(np.max(np.abs(dh))), "e_ref": float(np.max(np.abs(dr))), "r_hip": float(np.sqrt(np.mean(dh * dh))),
            "r_ref": float(np.sqrt(np.mean(dr * dr))), "fl": 2.0 ** -23 * float(np.max(np.abs(t64)))}


def measure(w, cfg, ids, scales, nw, got, sid=None, stages="EDRFG"):
    """Figures per stage tensor of one utterance, plus the f64 truths of stages D and R that the exact checks need. `stages`:
    the stages computed (a long utterance of a batched call leaves its flow and generator out: their f64 truths cost minutes)."""
    nz = got["noise_z"]
    C = cfg.inter
    t = {}
    for dt in (torch.float64, torch.float32):
        d = {}
        for st in stages:
            d.update(_truth(w, cfg, st, dt, ids, scales, nw, nz, got, sid))
        t[dt] = d
    t64, t32 = t[torch.float64], t[torch.float32]
    hip = {"x_enc": got["x_enc"], "m_p": got["stats"][:C], "logs_p": got["stats"][C:], "logw": got["logw"], "z": got["z"],
           "audio": got["audio"]}
    return {s: figures(hip[s], t64[s], t32[s]) for s in STAGES if s in t64}, t64


def check_gates(fig, gates, what):
    """e_hip <= K e_ref + fl and r_hip <= K r_ref per stage tensor; every figure is printed before anything is asserted."""
    bad = []
    for s in STAGES:
        if s not in fig:                   # a stage left out of this utterance (check_call's `stages`)
            continue
        f, K = fig[s], gates[s]
        print(f"{what} {s}: e_hip {f['e_hip']:.3e} e_ref {f['e_ref']:.3e} ratio {f['e_hip'] / max(f['e_ref'], 1e-300):.2f} | "
              f"r_hip {f['r_hip']:.3e} r_ref {f['r_ref']:.3e} ratio {f['r_hip'] / max(f['r_ref'], 1e-300):.2f} | fl {f['fl']:.2e} K {K}")
        if K is None:                      # printed with the rest, gated by the caller (a split matrix mode)
            continue
        if not (f["e_hip"] <= K * f["e_ref"] + f["fl"] and f["r_hip"] <= K * f["r_ref"]):
            bad.append((s, K, f))
    assert not bad, (what, bad)


def check_durations(got, t64, what, alone):
    """`alone`: the f64 w of the oracle alone (stage D from the oracle's own f64 x_enc): the seeds are chosen to keep it
    ORACLE_MARGIN from every integer, so that an engine x_enc that is 1e-6 off cannot break the precondition below."""
    v = t64["w"]
    T = v.size
    assert got["durations"].shape == (T,)
    dist = np.abs(v - np.round(v)) / np.maximum(1.0, v)
    da = np.abs(alone - np.round(alone)) / np.maximum(1.0, alone)
    print(f"{what} durations: the f64 w stays {dist.min():.3e} (relative) from an integer over {T} ids, the oracle alone {da.min():.3e}")
    assert np.all(da >= ORACLE_MARGIN), (what, "the seed does not keep the oracle alone away from an integer", float(da.min()))
    assert np.all(dist > CEIL_FLIP), (what, "the truth itself is too close to an integer", int(np.argmin(dist)), float(dist.min()))
    want = np.ceil(v).astype(np.int64)
    assert np.array_equal(got["durations"], want), (what, np.flatnonzero(got["durations"] != want)[:8])


def check_regulator(got, t64, what):
    d = got["durations"]
    Fr = max(int(d.sum()), 1)
    assert got["frames"] == Fr == t64["frames"] and got["z_p"].shape == t64["z_p"].shape == (got["stats"].shape[0] // 2, Fr), what
    want_id = np.repeat(np.arange(d.size), d) if d.sum() > 0 else np.full(1, -1)
    assert np.array_equal(t64["frame_id"], want_id), what          # generate_path's assignment is the plain repeat
    m, n = t64["z_p_m"], t64["z_p_n"]
    err = np.abs(got["z_p"].astype(np.float64) - (m + n))
    bound = 8 * 2.0 ** -24 * (np.abs(m) + np.abs(n))
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what} z_p: worst |d| / bound {worst:.3f} over {err.size} elements")
    assert np.all(err <= bound), (what, worst, np.argwhere(err > bound)[:4])


def check_call(target, vname, ids, scales, sids, nw, got, route, mode="f32", wseed=1234, gated=STAGES, k_case=None, stages=None):
    """Every check of one compared call, on every utterance of it; returns the figures per utterance. `scales`: one triple,
    or one per utterance ([B][3]: each utterance against the truth of its own). `gated`: the stage tensors under the K gates
    (a split matrix mode gates z and audio by truth_gates instead). `k_case`: {stage: K}, or {(utterance, stage): K}
    for one utterance of a batched call, of this case alone where its measured ratio asks for more than GATES (the profile file
    of the target's path says why). `stages`: {utterance: the stages
    checked on it} where that is not all of "EDRFG" (an utterance too long for its f64 flow and generator: "ED")."""
    cfg, w = voice(vname, wseed)
    lens = [len(s) for s in ids]
    figs = []
    for b in range(len(ids)):
        what = f"[{target} {vname} {lens} {route} {mode} utt {b}]"
        sid = None if sids is None else sids[b]
        g = got[b]
        assert np.array_equal(g["noise_w"], nw[b][:, :lens[b]]), what
        sc = tuple(float(x) for x in (scales[b] if np.ndim(scales) == 2 else scales))
        todo = (stages or {}).get(b, "EDRFG")
        assert "E" in todo and "D" in todo, todo
        fig, t64 = measure(w, cfg, ids[b], sc, nw[b], g, sid, todo)
        for s in STAGES:
            if s in fig:
                f = fig[s]
                ROWS.append((target, vname, lens, route, mode, b, s, f["e_hip"], f["e_ref"], f["r_hip"], f["r_ref"]))
        alone = _truth(w, cfg, "D", torch.float64, ids[b], sc, nw[b], None, {"x_enc": t64["x_enc"]}, sid)["w"]
        check_durations(g, t64, what, alone)
        if "R" in todo:
            check_regulator(g, t64, what)
        K = dict(GATES[target])
        for key, k in (k_case or {}).items():          # a stage, or (utterance, stage)
            if not isinstance(key, tuple):
                K[key] = k
            elif key[0] == b:
                K[key[1]] = k
        check_gates(fig, {s: (K[s] if s in gated else None) for s in STAGES}, what)
        figs.append(fig)
    return figs


def require(names, wanted, what):
    """Every entry of `wanted` -- a name, or a prefix ending in '<' or ',' -- was launched."""
    missing = [n for n in wanted if not (n in names or (n[-1] in "<," and any(x.startswith(n) for x in names)))]
    assert not missing, (what, missing, sorted(names))


def print_table(target):
    print(f"\n| target | voice | ids | route | mode | utt | stage | e_hip | e_ref | ratio | r_hip | r_ref | ratio |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for tg, v, lens, route, mode, b, s, eh, er, rh, rr in ROWS:
        if tg == target:
            print(f"| {tg} | {v} | {lens} | {route} | {mode} | {b} | {s} | {eh:.2e} | {er:.2e} | {eh / max(er, 1e-300):.2f} | {rh:.2e} | "
                  f"{rr:.2e} | {rh / max(rr, 1e-300):.2f} |")
    worst = {}
    for tg, v, lens, route, mode, b, s, eh, er, rh, rr in ROWS:
        if tg == target and mode == "f32":
            k = (s, route)
            a = worst.get(k, (0.0, 0.0))
            worst[k] = (max(a[0], eh / max(er, 1e-300)), max(a[1], rh / max(rr, 1e-300)))
    print("\n| stage | route | worst max ratio | worst rms ratio |\n|---|---|---|---|")
    for (s, route), (a, b) in sorted(worst.items()):
        print(f"| {s} | {route} | {a:.2f} | {b:.2f} |")
