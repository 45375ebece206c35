"""CPU (emulator) twin of tests/test_gpu_one_utterance_truth.py: the small-call kernels stage by stage against f64 truths
(tests/one_utterance_truth_case.py has the checks and the gates; profiles/one_utterance_truth.md the measured ratios).

The voices: the 192-channel tiny voice of test_emulated_192_channel_small_call_kernels, whose stage A and flow take the
4-column kernels of the medium / high qualities (PIPER_HIP_COL4=1) or their 16-column forms (=0), and the three tiny voices
as they are. The emulator has no graphs, so every case is one profiled call with injected noise; it rounds the f32
accumulator after every product of an MFMA, so its ratios against the oracle's f32 run are its own (GATES["emu"])."""
import os
import subprocess

import numpy as np
import pytest

import one_utterance_truth_case as U
from piper_amd import _lib as L

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
COL4 = {"1": {"attn4_kernel<96,false>", "colchain4_kernel<false>", "lngemm4_kernel", "dds_layer4_kernel", "ffn_kernel"},
        "0": {"attn_kernel<96>", "colchain_kernel<6>", "lngemm_kernel<6>", "dds_layer16_kernel<6>"}}
TINY = {"tiny": 1234, "tiny-high": 7, "tiny-ms": 5}          # weight seeds of tests/test_matrix_truth_emu.py


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()
    U.print_table("emu")          # (with -s: the figures of the cases that ran in this process, for profiles/one_utterance_truth.md)


def _case(lib, vname, lens, seed, env, route, wseed=1234, sids=None, mode="f32", gated=U.STAGES, k_case=None):
    cfg, _ = U.voice(vname, wseed)
    ids, nw, nz = U.batch_inputs(cfg, lens, seed)
    eng = U.engine_for(vname, env, lib=lib, wseed=wseed)
    got, names = U.run(eng, ids, U.SCALES, sids, nw, nz)
    print(f"[emu {vname} {lens} {route} {mode}] kernels: {sorted(names)}")
    for b, g in enumerate(got):
        assert np.array_equal(g["noise_z"], nz[b][:, :g["frames"]]), b
    figs = U.check_call("emu", vname, ids, U.SCALES, sids, nw, got, route, mode, wseed=wseed, gated=gated, k_case=k_case)
    return got, names, figs


@pytest.mark.parametrize("lens", [[5], [9, 31]])
@pytest.mark.parametrize("col4", ["0", "1"])
def test_192_channel_small_call_kernels_stage_by_stage(emu_lib, col4, lens):
    """5 ids: one full and one partial 4-column tile; 9 and 31: ragged, one id past two tiles and one short of eight. Seed 5
    keeps the oracle's own durations 3.7e-2 (5 ids), 3.9e-3 (9) and 2.4e-3 (31) from an integer."""
    _, names, _ = _case(emu_lib, "tiny192", lens, 5, {"PIPER_HIP_COL4": col4}, f"COL4={col4}")
    U.require(names, COL4[col4] | {"regulate_kernel", "duration_kernel"}, (col4, lens))
    assert not COL4["1" if col4 == "0" else "0"] & set(names), sorted(names)


@pytest.mark.parametrize("preset", sorted(TINY))
def test_tiny_voices_stage_by_stage(emu_lib, preset):
    """tiny, tiny-high (ResBlock1) and tiny-ms (speakers 1 and 3: dp.cond and the WN / generator conditioning) at 9 and 4 ids;
    seed 21 keeps the oracle's own durations >= 3.6e-3 from an integer on all three. tiny-high alone takes K = 16 on logw: its
    4-id utterance sits at 5.67 times an oracle f32 error that happens to be small there (profiles/one_utterance_truth.md)."""
    sids = [1, 3] if preset.endswith("-ms") else None
    _, names, _ = _case(emu_lib, preset, [9, 4], 21, {}, "default", wseed=TINY[preset], sids=sids,
                        k_case={"logw": 16} if preset == "tiny-high" else None)
    U.require(names, {"embed_kernel", "attn_kernel<", "regulate_kernel", "duration_kernel", "pcm16_kernel"}, preset)
    assert ("cond_kernel" in names) == (sids is not None), sorted(names)


def test_one_split_mode_on_flow_and_generator(emu_lib):
    """f16x3 on the tiled kernels (PIPER_HIP_SPLITK_MAX=0): everything in front of the flow is the f32 run's bit for bit and
    meets the f32 gates; z and audio meet truth_gates against the f32 run's error."""
    env = {"PIPER_HIP_SPLITK_MAX": 0}
    f32, _, ffig = _case(emu_lib, "tiny", [9, 4], 21, env, "SPLITK_MAX=0")
    got, names, fig = _case(emu_lib, "tiny", [9, 4], 21, dict(env, PIPER_HIP_MATRIX="f16x3"), "SPLITK_MAX=0", mode="f16x3",
                            gated=("x_enc", "m_p", "logs_p", "logw"))
    U.require(names, {"conv_split_kernel<1,", "mrf_split_kernel<1,"}, "f16x3")
    for b in range(2):
        for k in ("x_enc", "stats", "logw", "durations", "z_p"):
            assert np.array_equal(got[b][k], f32[b][k]), (b, k)
        for s in ("z", "audio"):
            # (the f32 run's own gate, against the f32 oracle on ITS input, was asserted by its _case; the mode's is relative to it)
            err = {"fl": fig[b][s]["fl"], "f32": ffig[b][s]["e_hip"], "f16x3": fig[b][s]["e_hip"]}
            assert U.truth_gates(err, "f16x3", "gauss"), (b, s, err)
