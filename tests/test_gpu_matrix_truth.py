"""The matrix modes against an f64 truth on an MI355X (run with -m gpu).

For each throughput shape -- configs[2] (high, 64 x 128 ids), configs[3]'s share (medium, 64 x 128) and x-low 12 x 128 --
and each weight family -- ``gauss``, ``heavy`` and ``rescaled`` (the gauss voice with channel gains 2^-5 .. 2^5 that the
next layer undoes exactly: piper_amd/weights.py rescale_channels) -- every matrix setting (f32, bf16x6, f16x3, bf16x3)
runs in the engine's default policy (medium also conv by conv: PIPER_HIP_BF3_MINF=0, PIPER_HIP_MRF_SPLIT=0). Sampled
utterances, the longest always among them, are decoded by ``oracle.decode`` in f64 and in torch f32 from the engine's
OWN z_p, so only the flow and generator arithmetic is compared. err(x) = max |d audio| against f64, fl = 2^-23 * peak.

The gates follow from the operand bits, not from a run:

    f32 HIP            <= 8 err(torch f32) + fl       two f32 summation orders
    bf16x6             <= 2 err(f32 HIP) + fl         exact operands, dropped products at 2^-24
    f16x3 gauss/heavy  <= 4 err(f32 HIP) + fl         22 of 24 significand bits
    bf16x3             <= 2^8 err(f32 HIP), < 2e-4    16 of 24 bits
    f16x3 rescaled     < 2e-4                         f16's exponent range: subnormal terms (measured, in the table)
    rescaled voice     f32 / bf16 modes bit-identical to the base voice
    overflow voice     f16x3 finite (activations beyond 131008 saturate the split)

The last test prints the table of err and rms per (preset, family, mode) kept in profiles/matrix_truth.md."""
import json

import numpy as np
import pytest
import torch

from oracle import vits_oracle as O
from piper_amd import weights as W

pytestmark = pytest.mark.gpu

MODES = ("f32", "bf16x6", "f16x3", "bf16x3")
SM = {"bf16x3": 0, "f16x3": 1, "bf16x6": 2}
PRODUCT_GATE = 2e-4
RESCALE_SEED = 11
# (preset, batch, seed, utterances compared with f64, route)
CASES = [("high", 64, 31, 4, "default"), ("medium", 64, 32, 8, "default"), ("medium", 64, 32, 8, "conv"),
         ("x-low", 12, 43, 8, "default")]
ROUTES = {"default": {}, "conv": {"PIPER_HIP_BF3_MINF": 0, "PIPER_HIP_MRF_SPLIT": 0}}
SCALES = (0.667, 1.0, 0.8)

_TRUTH = {}       # oracle.content_key(weights, z_p, sid, dtype) -> decoded audio: shared by every mode and family
_ROWS = []        # (preset, route, family, mode, err, rms, torch err, torch rms)


def _engine(monkeypatch, cfg, w, env):
    from piper_amd import _lib as L
    from piper_amd.engine import Engine
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    return Engine(blob=W.pack_blob(cfg, w), device=0)


def _run(monkeypatch, cfg, w, mode, route, ids, nw, nz):
    eng = _engine(monkeypatch, cfg, w, dict(ROUTES[route], PIPER_HIP_MATRIX=mode, PIPER_HIP_DEBUG_KEEP=1))
    eng.profile_enable(2)
    r = eng.synthesize_batch(ids, SCALES, noise_w=nw, noise_z=nz)
    names = {row["name"] for row in eng.profile()[5:] if row["launches"]}
    out = {"audio": [a.copy() for a in r.audio], "frames": np.asarray(r.frames).copy(), "durs": eng.durations().copy(),
           "zp": [eng.debug_tensor("z_p", b) for b in range(len(ids))]}
    eng.close()
    if mode != "f32":
        assert any(n.startswith(f"conv_split_kernel<{SM[mode]},") for n in names), (mode, sorted(names))
    return out


def _truth(w, cfg, zp, dtype):
    key = O.content_key(w, zp, None, str(dtype))
    if key not in _TRUTH:
        _TRUTH[key] = O.decode(w, cfg, zp, dtype=dtype).astype(np.float64)
    return _TRUTH[key]


def _inputs(cfg, B, seed):
    ids = [W.synthetic_phoneme_ids(128, 100 * seed + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(B)]
    rng = np.random.default_rng(seed)
    nw = rng.standard_normal((B, 2, 128)).astype(np.float32)
    nz = rng.standard_normal((B, cfg.inter, 6 * 128 + 64)).astype(np.float32)
    return ids, nw, nz


@pytest.mark.parametrize("preset,B,seed,nsample,route", CASES)
def test_matrix_modes_against_f64_truth(monkeypatch, preset, B, seed, nsample, route):
    cfg = W.preset(preset)
    base = W.synthetic_weights(cfg, 1234)
    fams = {"gauss": base, "heavy": W.synthetic_weights(cfg, 4321, family="heavy"),
            "rescaled": W.rescale_channels(cfg, base, RESCALE_SEED)}
    ids, nw, nz = _inputs(cfg, B, seed)
    runs = {}
    for fam, w in fams.items():
        for m in MODES:
            runs[fam, m] = _run(monkeypatch, cfg, w, m, route, ids, nw, nz)
    ref = runs["gauss", "f32"]
    frames = ref["frames"]
    longest = int(np.argmax(frames))
    sample = sorted({longest} | set(range(0, B, max(1, B // nsample))[:nsample - 1]))
    for fam in fams:
        for m in MODES:
            r = runs[fam, m]
            # the modes (and the rescaling) must not touch anything in front of the flow
            assert np.array_equal(r["durs"], runs[fam, "f32"]["durs"]), (fam, m)
            for b in range(B):
                assert np.array_equal(r["zp"][b], runs[fam, "f32"]["zp"][b]), (fam, m, b)
            if fam == "rescaled" and m != "f16x3":       # a power of two commutes with f32 and bf16 rounding
                for b in range(B):
                    assert np.array_equal(r["audio"][b], runs["gauss", m]["audio"][b]), (m, b)
    for fam, w in fams.items():
        tw = base if fam == "rescaled" else w            # the same function (tests/test_matrix_truth_emu.py): one truth
        errs = {m: [] for m in MODES + ("torch",)}
        sq = {m: [0.0, 0] for m in MODES + ("torch",)}
        for b in sample:
            zp = runs[fam, "f32"]["zp"][b]
            t = _truth(tw, cfg, zp, torch.float64)
            tf = _truth(tw, cfg, zp, torch.float32)
            fl = 2.0 ** -23 * float(np.max(np.abs(t)))
            e = {"torch": float(np.max(np.abs(tf - t)))}
            sq["torch"][0] += float(np.sum((tf - t) ** 2)); sq["torch"][1] += t.size
            for m in MODES:
                a = runs[fam, m]["audio"][b].astype(np.float64)
                assert a.shape == t.shape
                e[m] = float(np.max(np.abs(a - t)))
                sq[m][0] += float(np.sum((a - t) ** 2)); sq[m][1] += t.size
            for m in e:
                errs[m].append(e[m])
            ctx = (preset, route, fam, b, e)
            assert e["f32"] <= 8 * e["torch"] + fl, ctx
            assert e["bf16x6"] <= 2 * e["f32"] + fl, ctx
            if fam == "rescaled":
                assert e["f16x3"] < PRODUCT_GATE, ctx
            else:
                assert e["f16x3"] <= 4 * e["f32"] + fl, ctx
            assert e["bf16x3"] <= 2 ** 8 * e["f32"] and e["bf16x3"] < PRODUCT_GATE, ctx
        for m in MODES:
            _ROWS.append((preset, route, fam, m, max(errs[m]), float(np.sqrt(sq[m][0] / sq[m][1])),
                          max(errs["torch"]), float(np.sqrt(sq["torch"][0] / sq["torch"][1])), len(sample)))
    # the overflow voice: activations far beyond f16's range at the inputs of ups[0] and of the first MRF stage
    ov = _run(monkeypatch, cfg, W.rescale_channels(cfg, base, RESCALE_SEED, overflow_log2=18), "f16x3", route, ids, nw, nz)
    assert np.array_equal(ov["durs"], ref["durs"])
    for b in range(B):
        assert np.all(np.isfinite(ov["audio"][b])), f"utterance {b}: non-finite f16x3 audio on the overflow voice"


def test_print_truth_table():
    assert _ROWS, "run with the cases above"
    print("\n| preset | route | family | mode | max err | rms err | torch f32 max err | torch f32 rms err | utterances |")
    print("|---|---|---|---|---|---|---|---|---|")
    for p, r, f, m, e, s, te, ts, n in _ROWS:
        print(f"| {p} | {r} | {f} | {m} | {e:.2e} | {s:.2e} | {te:.2e} | {ts:.2e} | {n} |")
