"""CPU (emulator) tests of the split matrix modes against an f64 truth, and on voices that only differ from a base voice by
exact powers of two (piper_amd/weights.py: rescale_channels).

The truth is ``oracle.decode`` in f64 on the engine's OWN prior sample z_p (PIPER_HIP_DEBUG_KEEP=1): the flow and the
generator, exactly the arithmetic the modes change, so a one-frame flip of a duration's ceil cannot make two runs
incomparable. Every case forces the tiled kernels (PIPER_HIP_SPLITK_MAX=0), runs the engine's default route and the
conv-by-conv route (PIPER_HIP_BF3_MINF=0, PIPER_HIP_MRF_SPLIT=0), and asserts from the level-2 profile that the split
kernels really ran: a comparison that silently ran the f32 kernels would pass for any split arithmetic."""
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import vits_oracle as O
from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine
from one_utterance_truth_case import truth_gates          # (shared with the one-utterance truth tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")

SM = {"bf16x3": 0, "f16x3": 1, "bf16x6": 2}           # PIPER_HIP_MATRIX -> the kernels' split mode template argument
ROUTES = {"default": {}, "conv": {"PIPER_HIP_BF3_MINF": "0", "PIPER_HIP_MRF_SPLIT": "0"}}
PRESETS = {"tiny": 1234, "tiny-high": 7, "tiny-ms": 5}
LENS = {"tiny": (9, 4), "tiny-high": (4,), "tiny-ms": (9, 4)}          # (the emulated ResBlock1 stages are the slow ones)
SCALES = (0.6, 1.0, 0.7)
PRODUCT_GATE = 2e-4          # max |d audio| of the f32 path's own parity gate
RESCALE_SEED = 11


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _inputs(cfg, Ts=(9, 4), seed=21):
    ids = [W.synthetic_phoneme_ids(T, i, id_max=cfg.n_vocab - 1) for i, T in enumerate(Ts)]
    rng = np.random.default_rng(seed)
    nw = rng.standard_normal((len(Ts), 2, max(Ts))).astype(np.float32)
    nz = rng.standard_normal((len(Ts), cfg.inter, 32 * max(Ts) + 64)).astype(np.float32)
    sids = [1, 3][:len(Ts)] if cfg.n_speakers > 1 else None
    return ids, nw, nz, sids


def _run(emu_lib, monkeypatch, cfg, w, mode, route, inputs):
    """One batched call in matrix mode `mode` on route `route`: audio, pcm, durations, z_p per utterance."""
    ids, nw, nz, sids = inputs
    for k in ("PIPER_HIP_BF3_MINF", "PIPER_HIP_MRF_SPLIT", "PIPER_HIP_MRF"):
        monkeypatch.delenv(k, raising=False)
    for k, v in ROUTES[route].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PIPER_HIP_SPLITK_MAX", "0")
    monkeypatch.setenv("PIPER_HIP_DEBUG_KEEP", "1")
    monkeypatch.setenv("PIPER_HIP_MATRIX", mode)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    eng.profile_enable(2)
    r = eng.synthesize_batch(ids, SCALES, sids=sids, noise_w=nw, noise_z=nz)
    names = {row["name"] for row in eng.profile()[5:] if row["launches"]}
    out = {"audio": [a.copy() for a in r.audio], "pcm": [p.copy() for p in r.pcm], "durs": eng.durations().copy(),
           "zp": [eng.debug_tensor("z_p", b) for b in range(len(ids))]}
    eng.close()
    if mode != "f32":
        sm = SM[mode]
        assert any(n.startswith(f"conv_split_kernel<{sm},") for n in names), (mode, route, sorted(names))
        fused = route == "default" and mode != "bf16x6"          # mrf_split_kernel: the two-term modes' fused stage
        assert any(n.startswith(f"mrf_split_kernel<{sm},") for n in names) == fused, (mode, route, sorted(names))
        if route == "conv":
            assert not any(n.startswith("mrf_") and "sum" not in n for n in names), sorted(names)
    return out


def _truth(w, cfg, zp, sid, dtype=torch.float64):
    return O.decode(w, cfg, zp, sid=sid, dtype=dtype)


def _err(a, t):
    assert a.shape == t.shape
    return float(np.max(np.abs(a.astype(np.float64) - t)))


@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_rescaled_voices_compute_the_same_function_in_f64(preset):
    """The construction itself: the base voice, its rescaled copy and the overflow copy give the same f64 audio (within
    1e-12 of the peak), while the rescaling really moved the channels (and the overflow copy's conv_pre output is far beyond
    f16's range). The gauss / heavy draws are unchanged by the new code: the same seed still gives the same bits."""
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, PRESETS[preset])
    assert all(np.array_equal(w[k], v) for k, v in W.synthetic_weights(cfg, PRESETS[preset]).items())
    r = W.rescale_channels(cfg, w, RESCALE_SEED)
    ov = W.rescale_channels(cfg, w, RESCALE_SEED, overflow_log2=18)
    assert sorted(r) == sorted(w) and all(r[k].dtype == np.float32 and r[k].shape == w[k].shape for k in w)
    moved = [k for k in w if not np.array_equal(w[k], r[k])]
    assert any(k.startswith("flow.flows.") for k in moved) and any(k.startswith("dec.") for k in moved)
    assert not any(k.startswith(("enc_p.", "dp.", "emb_g")) or ".cond_layer." in k for k in moved), moved
    rng = np.random.default_rng(3)
    zp = rng.standard_normal((cfg.inter, 17)).astype(np.float32)
    sid = 2 if cfg.n_speakers > 1 else None
    t = _truth(w, cfg, zp, sid)
    peak = float(np.max(np.abs(t)))
    assert peak > 0.01
    for v in (r, ov):
        assert np.max(np.abs(_truth(v, cfg, zp, sid) - t)) <= 1e-12 * peak
    wt = O.to_torch(ov, torch.float64)
    pre = O._conv(wt, "dec.conv_pre", torch.as_tensor(zp, dtype=torch.float64)[None], padding=3)
    assert float(pre.abs().max()) > 4 * 131024.0


@pytest.mark.parametrize("preset", sorted(PRESETS))
@pytest.mark.parametrize("mode,route", [("f32", "default")] + [(m, r) for m in ("bf16x3", "bf16x6") for r in sorted(ROUTES)])
def test_f32_and_bf16_modes_are_bit_identical_on_rescaled_voices(emu_lib, monkeypatch, preset, mode, route):
    """A power of two commutes with f32 and bf16 rounding (bf16 has f32's exponent range), so the f32 kernels and the
    bf16 split modes must give the SAME bits on the base voice, its rescaled copy (channel gains 2^-5 .. 2^5) and the
    overflow copy (stage 0 times another 2^18). A mode that dropped a term or rounded differently per channel would not
    be caught by a tolerance this tight; the f32 path does not depend on the route, so it runs once."""
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, PRESETS[preset])
    inputs = _inputs(cfg, LENS[preset])
    base = _run(emu_lib, monkeypatch, cfg, w, mode, route, inputs)
    for ovf in (None, 18):
        v = W.rescale_channels(cfg, w, RESCALE_SEED, overflow_log2=ovf)
        o = _run(emu_lib, monkeypatch, cfg, v, mode, route, inputs)
        assert np.array_equal(o["durs"], base["durs"])
        for b in range(len(inputs[0])):
            assert np.array_equal(o["zp"][b], base["zp"][b])
            assert np.array_equal(o["audio"][b], base["audio"][b]), (ovf, b, np.max(np.abs(o["audio"][b] - base["audio"][b])))
            assert np.array_equal(o["pcm"][b], base["pcm"][b])


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_f16x3_on_rescaled_and_overflow_voices(emu_lib, monkeypatch, preset, route):
    """f16x3 is the one mode the rescaling may change (f16's exponent range). On the rescaled voice it must stay inside the
    product gate against the f64 truth. On the overflow voice (activations near 2^24 at the inputs of ups[0] and of the
    first MRF stage) both terms of the split saturate: the audio is wrong but finite, the durations are the f32 path's,
    and the PCM is the int16 conversion of that audio. (Before the split saturated its low term, f16(v - 65504) was inf
    for |v| >= 131024 and one such activation turned the utterance into NaN.)"""
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, PRESETS[preset])
    inputs = _inputs(cfg, LENS[preset])
    ids, nw, _, sids = inputs
    rs = _run(emu_lib, monkeypatch, cfg, W.rescale_channels(cfg, w, RESCALE_SEED), "f16x3", route, inputs)
    wt = O.to_torch(w)
    for b in range(len(ids)):
        sid = None if sids is None else sids[b]
        assert np.array_equal(rs["durs"][sum(len(x) for x in ids[:b]):][:len(ids[b])],
                              O.durations_only(wt, cfg, ids[b], SCALES, nw[b], sid))
        e = _err(rs["audio"][b], _truth(w, cfg, rs["zp"][b], sid))
        assert e < PRODUCT_GATE, (b, e)
    ov = _run(emu_lib, monkeypatch, cfg, W.rescale_channels(cfg, w, RESCALE_SEED, overflow_log2=18), "f16x3", route, inputs)
    assert np.array_equal(ov["durs"], rs["durs"])
    for b in range(len(ids)):
        assert np.array_equal(ov["zp"][b], rs["zp"][b])
        assert np.all(np.isfinite(ov["audio"][b])), f"utterance {b}: non-finite f16x3 audio on the overflow voice"
        assert np.array_equal(ov["pcm"][b], O.audio_float_to_int16(ov["audio"][b]))


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("family", ["gauss", "heavy"])
def test_split_modes_against_the_f64_truth(emu_lib, monkeypatch, family, route):
    """Every mode against f64 on the engine's own z_p, gated from its operand bits relative to the f32 kernels (which are
    gated against the oracle's f32 run): bf16x6 (all 24 bits) within 3x of f32 (truth_gates), f16x3 (22 bits) within 4x, bf16x3 (16
    bits) within 2^8x -- each plus one f32 ulp of the peak. A bf16x6 that lost its third term, or an f16x3 whose low term
    lost bits, lands at bf16x3's error and fails."""
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 4321, family=family)
    inputs = _inputs(cfg, Ts=(8, 3), seed=23)
    runs = {m: _run(emu_lib, monkeypatch, cfg, w, m, route, inputs) for m in ("f32", "bf16x6", "f16x3", "bf16x3")}
    for b in range(len(inputs[0])):
        zp = runs["f32"]["zp"][b]
        for m in runs:
            assert np.array_equal(runs[m]["zp"][b], zp) and np.array_equal(runs[m]["durs"], runs["f32"]["durs"])
        t = _truth(w, cfg, zp, None)
        err = {"torch": _err(_truth(w, cfg, zp, None, torch.float32), t), "fl": 2.0 ** -23 * float(np.max(np.abs(t)))}
        for m in runs:
            err[m] = _err(runs[m]["audio"][b], t)
        for m in runs:
            assert truth_gates(err, m, family), (m, b, err)
