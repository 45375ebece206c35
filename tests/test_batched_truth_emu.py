"""CPU (emulator) twin of tests/test_gpu_batched_truth.py: ragged batched calls of five to seven utterances stage by stage
against f64 truths, every check of tests/one_utterance_truth_case.py on EVERY utterance of the call (gates: its
GATES["emu-batched"]; measured ratios: profiles/batched_truth.md).

The emulator has no graphs: every case is one profiled call with injected noise. Each batch holds utterances of 1, 2 and 3
ids (the attention's clipped relative-position window, a row that owns less than one tile) between longer ones, so that the
utterance index on blockIdx.y / blockIdx.z runs past 1 with a short utterance in the middle; one holds an utterance of 65
frames, one column past a 64-column tile. Duration-noise seeds keep the oracle's own f64 durations this far (relative) from
an integer: tiny [2, 9, 1, 5, 3, 9] seed 2 5.4e-2, with mixed scales 3.8e-2; tiny [2, 44, 1, 5, 3, 9] seed 8 1.6e-2;
tiny-high [2, 9, 1, 5, 3] seed 3 3.2e-2; tiny-ms [1, 2, 3, 9, 5, 7] seed 2 9.4e-3; tiny192 [2, 9, 1, 5, 3] seed 6 1.6e-2."""
import os
import subprocess

import numpy as np
import pytest

import one_utterance_truth_case as U
from piper_amd import _lib as L

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
TARGET = "emu-batched"
RAGGED, SEED = [2, 9, 1, 5, 3, 9], 2
# the tiled forms of a batch too small to reach them by itself, the one-tap convs with them
TILED = {"conv1x1_kernel<1>", "conv_mfma_kernel<1,4,2,1,16,true,64>", "conv_mfma_kernel<2,2,1,1,16,false,64>",
         "conv_mfma_kernel<1,4,1,1,16,false,64>"}
SPLITK = {"conv_splitk_kernel<", "conv_splitk16_kernel<", "conv_splitk_group_kernel<", "gate4_kernel"}
# {(voice, utterances, route): k_case}: logw of the utterances whose measured ratio is above 4 -- the smallest power of two at
# least twice the ratio (profiles/batched_truth.md: a handful of values against an oracle f32 error that happens to be small)
_R6 = {(0, "logw"): 16, (3, "logw"): 16}
K_CASE = {("tiny", 6, "default"): _R6, ("tiny", 6, "ATTN_LONG=1"): _R6, ("tiny", 6, "mixed scales"): {(0, "logw"): 16},
          ("tiny", 6, "SPLITK_MAX=0"): {(4, "logw"): 32}, ("tiny", 6, "SPLITK_MAX=0,TPB=3"): {(4, "logw"): 32}, ("tiny-ms", 6, "default"): {(5, "logw"): 16},
          ("tiny192", 5, "default"): {(2, "logw"): 16}, ("tiny", 5, "SPLITK_MAX=0"): {(2, "logw"): 32}}
K_CASE.update({("tiny", 6, f"MRF_OU={ou}"): _R6 for ou in (1, 2, 3, 4)})


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()
    U.print_table(TARGET)          # (with -s: the figures of the cases that ran in this process, for profiles/batched_truth.md)


def _case(lib, vname, lens, seed, env, route, wseed=1234, scales=U.SCALES, sids=None, mode="f32", gated=U.STAGES):
    cfg, _ = U.voice(vname, wseed)
    ids, nw, nz = U.batch_inputs(cfg, lens, seed)
    eng = U.engine_for(vname, env, lib=lib, wseed=wseed)
    got, names = U.run(eng, ids, scales, sids, nw, nz)
    print(f"[{TARGET} {vname} {lens} {route} {mode}] frames {[g['frames'] for g in got]} kernels: {sorted(names)}")
    for b, g in enumerate(got):
        assert np.array_equal(g["noise_z"], nz[b][:, :g["frames"]]), b
    figs = U.check_call(TARGET, vname, ids, scales, sids, nw, got, route, mode, wseed=wseed, gated=gated,
                        k_case=K_CASE.get((vname, len(lens), route)))
    return got, names, figs


def _gone(names, gone, what):
    left = [x for x in names for n in gone if x == n or (n[-1] in "<," and x.startswith(n))]
    assert not left, (what, left)


def test_ragged_batch_default_policy(emu_lib):
    """Six utterances of 2, 9, 1, 5, 3 and 9 ids (two equal lengths) on the tiny voice, as the engine routes them."""
    _, names, _ = _case(emu_lib, "tiny", RAGGED, SEED, {}, "default")
    U.require(names, {"embed_kernel", "attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>", "duration_kernel", "regulate_kernel",
                      "conv_splitk_kernel<2,true,", "conv_splitk_kernel<1,false,", "mrf_kernel<32,", "pcm16_kernel"}, "default")


def test_tiled_forms_and_one_tap_convs(emu_lib):
    """PIPER_HIP_SPLITK_MAX=0: the gate conv, the plain convs and the up-convs through the tiled kernel and the one-tap convs
    through conv1x1_kernel<1>, on a batch whose second utterance has 65 frames: one column in the second 64-column tile,
    between utterances that own a few columns of their first."""
    got, names, _ = _case(emu_lib, "tiny", [2, 44, 1, 5, 3, 9], 8, {"PIPER_HIP_SPLITK_MAX": 0}, "SPLITK_MAX=0")
    assert got[1]["frames"] == 65, [g["frames"] for g in got]
    U.require(names, TILED | {"mrf_kernel<32,", "duration_kernel"}, "SPLITK_MAX=0")
    _gone(names, SPLITK, "SPLITK_MAX=0")


def test_several_column_tiles_per_workgroup(emu_lib):
    """PIPER_HIP_TPB=3 from PIPER_HIP_SPLITK_MAX=0: the tiled kernel walks the 65-frame utterance's two column tiles (and the up-convs'
    further ones) in one workgroup, slab after slab, beside utterances that end inside their first. It renames no kernel."""
    env = {"PIPER_HIP_SPLITK_MAX": 0, "PIPER_HIP_TPB": 3}
    got, names, _ = _case(emu_lib, "tiny", [2, 44, 1, 5, 3, 9], 8, env, "SPLITK_MAX=0,TPB=3")
    assert got[1]["frames"] == 65, [g["frames"] for g in got]
    U.require(names, TILED, "TPB=3")
    _gone(names, SPLITK, "TPB=3")


@pytest.mark.parametrize("ou", [1, 2, 3, 4])
def test_fused_mrf_stage_at_each_output_unit_count(emu_lib, ou):
    """mrf_kernel<32, OU, 1> at every OU the 32-channel stages admit, on the ragged batch (windows that start before an
    utterance of one frame and end behind it)."""
    _, names, _ = _case(emu_lib, "tiny", RAGGED, SEED, {"PIPER_HIP_MRF_OU": ou}, f"MRF_OU={ou}")
    U.require(names, {f"mrf_kernel<32,{ou},1>"}, ou)
    _gone(names, {f"mrf_kernel<32,{k}," for k in (1, 2, 3, 4) if k != ou}, ou)


def test_attention_with_score_slabs_in_global_memory(emu_lib):
    """PIPER_HIP_ATTN_LONG=1: attn_long_kernel<0> in place of attn_kernel<0> (softmax over an utterance's own length, 1 .. 9)."""
    _, names, _ = _case(emu_lib, "tiny", RAGGED, SEED, {"PIPER_HIP_ATTN_LONG": 1}, "ATTN_LONG=1")
    U.require(names, {"attn_long_kernel<0>"}, "ATTN_LONG=1")
    _gone(names, {"attn_kernel<"}, "ATTN_LONG=1")


def test_mixed_scales_per_utterance(emu_lib):
    """One {noise_scale, length_scale, noise_w} triple per utterance (length_scale 0.75 .. 1.3): each utterance against the
    truth of its own triple; duration_kernel and regulate_kernel read utterance b's."""
    _, names, _ = _case(emu_lib, "tiny", RAGGED, SEED, {}, "mixed scales", scales=U.MIXED_SCALES[:len(RAGGED)])
    U.require(names, {"duration_kernel", "regulate_kernel"}, "mixed scales")


def test_distinct_speakers_per_utterance(emu_lib):
    """tiny-ms, speakers 3, 1, 0, 2, 1, 3 (two of them repeated): cond_kernel and the conditioning rows by utterance."""
    _, names, _ = _case(emu_lib, "tiny-ms", [1, 2, 3, 9, 5, 7], 2, {}, "default", wseed=5, sids=[3, 1, 0, 2, 1, 3])
    U.require(names, {"cond_kernel", "duration_kernel", "regulate_kernel", "mrf_kernel<32,"}, "tiny-ms")


@pytest.mark.parametrize("vname,wseed,seed,env,route,appear,gone", [
    ("tiny-high", 7, 3, {}, "default", {"attn_kernel<0>", "duration_kernel", "regulate_kernel"}, set()),
    ("tiny-high", 7, 3, {"PIPER_HIP_SPLITK_MAX": 0}, "SPLITK_MAX=0", {"conv1x1_kernel<1>", "conv_mfma_kernel<1,4,2,1,16,true,64>"}, SPLITK),
    ("tiny192", 1234, 6, {}, "default", {"attn4_kernel<96,false>", "colchain4_kernel<false>", "lngemm4_kernel", "dds_layer4_kernel",
                                         "ffn_kernel", "duration_kernel", "regulate_kernel"}, set()),
    ("tiny192", 1234, 6, {"PIPER_HIP_COL4": 0, "PIPER_HIP_SPLITK_MAX": 0}, "COL4=0,SPLITK_MAX=0",
     {"attn_kernel<96>", "colchain_kernel<6>", "lngemm_kernel<6>", "dds_layer16_kernel<6>", "conv1x1_kernel<1>"},
     SPLITK | {"colchain4_kernel<", "lngemm4_kernel", "dds_layer4_kernel"})])
def test_resblock1_and_192_channel_voices(emu_lib, vname, wseed, seed, env, route, appear, gone):
    """tiny-high (ResBlock1 generator) and the 192-channel tiny voice (the 4-column chains of the medium / high qualities, and
    their 16-column forms with the tiled kernels behind them) on five utterances of 2, 9, 1, 5 and 3 ids."""
    _, names, _ = _case(emu_lib, vname, [2, 9, 1, 5, 3], seed, env, route, wseed=wseed)
    U.require(names, appear, (vname, route))
    _gone(names, gone, (vname, route))


def test_one_split_mode_on_a_ragged_batch(emu_lib):
    """f16x3 on the tiled kernels (PIPER_HIP_SPLITK_MAX=0), five utterances: everything in front of the flow is the f32 run's
    bit for bit and meets the f32 gates; z and audio meet truth_gates against the f32 run's error, on every utterance."""
    env, lens = {"PIPER_HIP_SPLITK_MAX": 0}, RAGGED[:5]
    f32, _, ffig = _case(emu_lib, "tiny", lens, SEED, env, "SPLITK_MAX=0")
    got, names, fig = _case(emu_lib, "tiny", lens, SEED, dict(env, PIPER_HIP_MATRIX="f16x3"), "SPLITK_MAX=0", mode="f16x3",
                            gated=("x_enc", "m_p", "logs_p", "logw"))
    U.require(names, {"conv_split_kernel<1,", "mrf_split_kernel<1,"}, "f16x3")
    for b in range(len(lens)):
        for k in ("x_enc", "stats", "logw", "durations", "z_p"):
            assert np.array_equal(got[b][k], f32[b][k]), (b, k)
        for s in ("z", "audio"):
            err = {"fl": fig[b][s]["fl"], "f32": ffig[b][s]["e_hip"], "f16x3": fig[b][s]["e_hip"]}
            print(f"[{TARGET} tiny {lens} SPLITK_MAX=0 f16x3 utt {b}] {s}: {err}")
            assert U.truth_gates(err, "f16x3", "gauss"), (b, s, err)
