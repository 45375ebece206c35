"""The batched path stage by stage against f64 truths on an MI355X (run with -m gpu): ragged calls of five to eight
utterances, every check of tests/one_utterance_truth_case.py -- the six stage tensors under K gates from the engine's own
input to each stage, every duration equal to the ceil of the f64 value, the z_p 8-ulp bound, the frame counts -- on EVERY
utterance of the call (gates: GATES["gpu-batched"]; measured ratios and the reason for every K: profiles/batched_truth.md).

The compared call. Five or more utterances are never one speculative graph: stage A (duration_kernel at its end), the
read-back of the frame counts, stage B, as two graphs. `run` (graph="two") calls twice with injected duration noise and the
engine's own prior noise -- first the same lengths with ids and noise reversed (an utterance of one id, which is its own
reverse: the next id and the negated noise), whose front-half buffers must differ from the compared call's -- asserts from
speculation_stats and graph_stats that nothing was speculative and graphs were replayed, reads every tensor back (the prior
noise included), and repeats the call under the level-2 profile with that noise injected: durations and z_p bit for bit, and
the kernel names are the repeat's. The long utterances (900 + 40 ids, 600 ids) are calls of one and two utterances, which
would be speculative: they run with PIPER_HIP_SPEC=0, which selects no kernel, so that they take the same two-graph path.

Shapes are the smallest that reach the form. Every batch holds utterances of 1, 2 and 3 ids (the attention's clipped
relative-position window; a row that owns less than one tile) BETWEEN longer ones, so a short utterance never sits at the
end of the index range. The default policy sends a gate conv to the tiled kernel and the one-tap convs to conv1x1_kernel<1>
from 96 tile workgroups on, which eight utterances reach when the longest has more than 384 frames: the first case therefore
has one utterance of 128 ids (396 frames) beside seven of at most 64.

Duration-noise seeds keep the oracle's own f64 durations this far (relative) from an integer: medium [2, 22, 1, 33, 128, 3,
33, 64] seed 10 8.0e-4 (frames 4, 65, 4, 116, 396, 12, 101, 189), with mixed scales seed 1 1.9e-3; medium [2, 40, 1, 21, 3]
seed 3 7.3e-3; high [2, 40, 1, 17, 3, 33] seed 5 7.8e-3; x-low [64, 1, 64, 2, 33, 3, 64, 64] seed 3 1.1e-3; tiny-ms [1, 2, 3,
9, 33, 20, 5, 12] seed 10 2.6e-3; x-low and tiny [20, 1, 33, 2, 3] seeds 2 and 6 3.3e-3 and 1.3e-2; medium [900, 40] seed 14
1.1e-3; medium [600] seed 36 1.0e-3.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import numpy as np
import pytest

import one_utterance_truth_case as U

pytestmark = pytest.mark.gpu

TARGET = "gpu-batched"
FRONT4 = {"colchain4_kernel<false>", "lngemm4_kernel", "ffn_kernel", "dds_layer4_kernel"}
TWO = {"embed_kernel", "duration_kernel", "regulate_kernel", "pcm16_kernel"}          # stage A ends in duration_kernel: no one-graph call
RAGGED8, SEED8 = [2, 22, 1, 33, 128, 3, 33, 64], 10
RAGGED5, SEED5 = [2, 40, 1, 21, 3], 3
# {(voice, utterances, route): k_case}: the utterances whose measured ratio is above 4 (profiles/batched_truth.md has each reason)
K_CASE = {         # all of them logw, all but one of utterances of 1 .. 9 ids: a few values against an oracle f32 error that happens to be near one ulp
    ("medium", 8, "mixed scales"): {(2, "logw"): 16}, ("tiny-ms", 8, "default"): {(2, "logw"): 16, (3, "logw"): 16},
    ("medium", 5, "PIPER_HIP_COLCHAIN=0"): {(0, "logw"): 16}, ("medium", 5, "PIPER_HIP_COLCHAIN=2,PIPER_HIP_COL4=0"): {(2, "logw"): 16},
    ("medium", 5, "PIPER_HIP_FUSE_DP=0"): {(2, "logw"): 16}, ("medium", 5, "PIPER_HIP_ATTN4=0"): {(1, "logw"): 16, (2, "logw"): 32},
    ("x-low", 5, "PIPER_HIP_ATTN_LONG=1"): {(4, "logw"): 16}, ("tiny", 5, "PIPER_HIP_ATTN_LONG=1"): {(1, "logw"): 16},
}

# (knob(s) flipped, the policy they are flipped from) on medium, RAGGED5
ROUTES = [("PIPER_HIP_CONV1X1=0", "PIPER_HIP_COLCHAIN=0,PIPER_HIP_SPLITK_MAX=0"), ("PIPER_HIP_COLCHAIN=0", ""),
          ("PIPER_HIP_COLCHAIN=2,PIPER_HIP_COL4=0", ""), ("PIPER_HIP_COL4=2", ""), ("PIPER_HIP_MRF=0", ""),
          ("PIPER_HIP_GROUP_TILED=0", "PIPER_HIP_MRF=0"), ("PIPER_HIP_MRF_OU=1", ""), ("PIPER_HIP_MRF_OU=2", ""),
          ("PIPER_HIP_MRF_OU=3", ""), ("PIPER_HIP_MRF_OU=4", ""), ("PIPER_HIP_MRF_TAIL=0", ""),
          ("PIPER_HIP_TPB=3", "PIPER_HIP_SPLITK_MAX=0"), ("PIPER_HIP_FUSE_DP=0", ""), ("PIPER_HIP_ATTN4=0", ""),
          ("PIPER_HIP_ATTNO=0", ""), ("PIPER_HIP_ATTN_LONG=1", "")]
# knob -> (kernels that must appear, kernels that must be gone) against the policy it is flipped from; a name, or a prefix
SELECTS = {
    "PIPER_HIP_CONV1X1=0": ({"conv_mfma_kernel<1,4,1,1,16,false,64>"}, {"conv1x1_kernel<1>"}),
    "PIPER_HIP_COLCHAIN=0": ({"ln_kernel", "attn_kernel<96>"}, {"lngemm4_kernel", "colchain4_kernel<true>", "ffn_kernel", "attn4_kernel<"}),
    "PIPER_HIP_COLCHAIN=2,PIPER_HIP_COL4=0": ({"colchain_kernel<6>", "lngemm_kernel<6>", "dds_layer16_kernel<6>", "attn_kernel<96>"},
                                              {"colchain4_kernel<", "lngemm4_kernel", "dds_layer4_kernel", "ffn_kernel", "attn4_kernel<"}),
    "PIPER_HIP_MRF=0": ({"conv_post_kernel", "mrf_sum_kernel", "conv_mfma_group_kernel<"}, {"mrf_kernel<"}),
    "PIPER_HIP_GROUP_TILED=0": (set(), {"conv_mfma_group_kernel<", "mrf_sum_kernel"}),
    "PIPER_HIP_MRF_TAIL=0": ({"conv_post_kernel"}, set()),
    "PIPER_HIP_FUSE_DP=0": ({"cf_pre_kernel", "scale_kernel", "spline_inverse_kernel"}, set()),
    "PIPER_HIP_ATTN4=0": ({"attno_kernel<96>"}, {"attn4_kernel<"}),
    "PIPER_HIP_ATTNO=0": ({"attn_kernel<96>"}, {"attn4_kernel<"}),
    "PIPER_HIP_ATTN_LONG=1": ({"attn_long_kernel<96>"}, {"attn4_kernel<"}),
}
# knobs that change no kernel name at this size: the kernels they steer must be there, the name set must be the base's
SAME = {"PIPER_HIP_COL4=2": FRONT4, "PIPER_HIP_TPB=3": {"conv_mfma_kernel<2,2,2,1,16,true,64>", "conv_mfma_kernel<2,2,1,1,16,false,64>"}}

_POLICY = {}         # policy -> (tensors, names, figures) on the medium voice, RAGGED5


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()
    U.print_table(TARGET)          # (with -s: the figures kept in profiles/batched_truth.md)


def _env(policy):
    return dict(kv.split("=") for kv in policy.split(",") if kv)


def _case(vname, lens, seed, route, env=None, scales=U.SCALES, sids=None, mode="f32", eng=None, gated=U.STAGES, stages=None):
    from piper_amd.engine import EngineError
    cfg, _ = U.voice(vname)
    ids, nw, _ = U.batch_inputs(cfg, lens, seed)
    try:
        e = eng or U.engine_for(vname, env)
        got, names = U.run(e, ids, scales, sids, nw, graph="two")
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {vname} {route}: {ex}", returncode=3)
    print(f"[{TARGET} {vname} {lens} {route} {mode}] frames {[g['frames'] for g in got]} kernels: {sorted(names)}")
    figs = U.check_call(TARGET, vname, ids, scales, sids, nw, got, route, mode, gated=gated, stages=stages,
                        k_case=K_CASE.get((vname, len(lens), route)))
    return got, names, figs


def _gone(names, gone, what):
    left = [x for x in names for n in gone if x == n or (n[-1] in "<," and x.startswith(n))]
    assert not left, (what, left)


def _medium5(policy=""):
    """The medium voice on RAGGED5 under `policy` ("KNOB=v,KNOB=v", "" = the default), run once per module."""
    if policy not in _POLICY:
        _POLICY[policy] = _case("medium", RAGGED5, SEED5, policy or "default", _env(policy))
    return _POLICY[policy]


def test_default_policy_ragged():
    """Medium, eight utterances of 2, 22, 1, 33, 128, 3, 33 and 64 ids: 1, 2 and 3 ids between longer ones, two equal lengths,
    the second utterance 65 frames (one column in its second 64-column tile), the fifth long enough (396 frames) that the
    default policy takes the tiled gate conv and conv1x1_kernel<1> for the whole call."""
    got, names, _ = _case("medium", RAGGED8, SEED8, "default")
    assert got[1]["frames"] == 65 and max(g["frames"] for g in got) > 384, [g["frames"] for g in got]
    U.require(names, TWO | FRONT4 | {"conv_mfma_kernel<2,2,2,1,16,true,64>", "conv1x1_kernel<1>", "mrf_kernel<64,", "mrf_kernel<32,",
                                     "attn4_kernel<96,false>"}, "default")
    _gone(names, {"gate4_kernel", "conv_splitk16_kernel<true,"}, "default")


def test_mixed_scales_per_utterance():
    """The same lengths, one {noise_scale, length_scale, noise_w} triple per utterance (length_scale 0.75 .. 1.4, the second
    utterance at 1.3): every utterance against the truth of its own triple."""
    sc = U.MIXED_SCALES[:len(RAGGED8)]
    assert sc[1, 1] == np.float32(1.3) and len({tuple(r) for r in sc.tolist()}) == len(RAGGED8)
    _, names, _ = _case("medium", RAGGED8, 1, "mixed scales", scales=sc)
    U.require(names, TWO | FRONT4 | {"mrf_kernel<64,", "mrf_kernel<32,"}, "mixed scales")


# what each of the other voices is there for: the ResBlock1 generator's grouped tiled launches with their sum (high); the
# 96-channel forms, 48-channel coupling halves and three 32-channel chunks (x-low; the 64 x 128 gate tile
# conv_mfma_kernel<1,4,2,1,16,true,64> needs more columns than eight utterances of 64 ids have: it stays with the B = 32
# parity test of tests/test_gpu_batched.py); the conditioning launch and per-utterance conditioning rows (tiny-ms)
OTHERS = {
    "high": ([2, 40, 1, 17, 3, 33], 5, None,
             TWO | FRONT4 | {"attn4_kernel<96,false>", "conv_mfma_group_kernel<", "mrf_sum_kernel", "mrf_kernel<32,"}),
    "x-low": ([64, 1, 64, 2, 33, 3, 64, 64], 3, None,
              TWO | {"attn_kernel<48>", "ln_kernel", "dds_layer16_kernel<3>", "conv_mfma_kernel<", "mrf_kernel<64,", "mrf_kernel<32,"}),
    "tiny-ms": ([1, 2, 3, 9, 33, 20, 5, 12], 10, [0, 1, 2, 3, 1, 2, 0, 3],
                TWO | {"cond_kernel", "attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>", "mrf_kernel<32,"}),
}


@pytest.mark.parametrize("vname", sorted(OTHERS))
def test_other_voices(vname):
    """high (six utterances of at most 40 ids), x-low (eight of at most 64), tiny-ms (eight, speakers 0 1 2 3 1 2 0 3: each
    its own, 1 and 2 and 3 repeated)."""
    lens, seed, sids, wanted = OTHERS[vname]
    _, names, _ = _case(vname, lens, seed, "default", sids=sids)
    U.require(names, wanted, vname)


@pytest.mark.parametrize("knob,base", ROUTES)
def test_forced_forms_compute_the_same_function(knob, base):
    """One knob flipped on five ragged utterances (2, 40, 1, 21 and 3 ids: 135, 72 and a few frames), from the default or from
    the policy that reaches the form: the same function, the same gates on every utterance. A knob that selects kernels must
    launch those of SELECTS and none of those it replaces; PIPER_HIP_MRF_OU must put the 32-channel stage, and up to 3 the
    64-channel stage, on that many output units and on no other; the two of SAME steer kernels without renaming them."""
    _, ref, _ = _medium5(base)
    _, names, _ = _medium5(",".join(x for x in (base, knob) if x))
    if knob in SAME:
        U.require(names, SAME[knob], knob)
        assert set(names) == set(ref), (knob, sorted(set(names) ^ set(ref)))
    elif knob.startswith("PIPER_HIP_MRF_OU="):
        ou = int(knob[-1])
        U.require(names, {f"mrf_kernel<32,{ou},1>"} | ({f"mrf_kernel<64,{ou},2>"} if ou <= 3 else {"mrf_kernel<64,"}), knob)
        _gone(names, {f"mrf_kernel<32,{k}," for k in (1, 2, 3, 4) if k != ou}, knob)
        _gone(names, {f"mrf_kernel<64,{k}," for k in (1, 2, 3) if k != ou and ou <= 3}, knob)
    else:
        appear, gone = SELECTS[knob]
        U.require(names, appear, knob)
        assert set(names) != set(ref) and not [n for n in appear if n in ref], (knob, sorted(ref))
        for n in gone:
            U.require(ref, {n}, (knob, "flipped from a policy that does not launch it"))
        _gone(names, gone, knob)


@pytest.mark.parametrize("vname,seed,wanted,gone", [("x-low", 2, "attn_long_kernel<48>", "attn_kernel<"), ("tiny", 6, "attn_long_kernel<0>", "attn_kernel<")])
def test_attention_score_slabs_in_global_memory_on_the_other_widths(vname, seed, wanted, gone):
    """PIPER_HIP_ATTN_LONG=1 on x-low and tiny (medium: ROUTES): five utterances of 20, 1, 33, 2 and 3 ids."""
    _, names, _ = _case(vname, [20, 1, 33, 2, 3], seed, "PIPER_HIP_ATTN_LONG=1", {"PIPER_HIP_ATTN_LONG": 1})
    U.require(names, {wanted}, vname)
    _gone(names, {gone}, vname)


def test_upconv_store_forms_are_bit_identical():
    """PIPER_HIP_CONVT_VEC=0 selects no kernel: the polyphase up-convs store their tile one 4-byte sample at a time. Both forms
    on fresh engines (the same run counter, so the same prior noise): every gate met by each on every utterance, the same
    {kernel: launches} map, and z and the audio of every utterance equal bit for bit."""
    runs = {}
    for route, env in (("default", {}), ("PIPER_HIP_CONVT_VEC=0", {"PIPER_HIP_CONVT_VEC": 0})):
        eng = U.engine_for("medium", env, fresh=True)
        try:
            runs[route] = _case("medium", RAGGED5, SEED5, route, eng=eng)
        finally:
            eng.close()
    (a, an, _), (b, bn, _) = runs["default"], runs["PIPER_HIP_CONVT_VEC=0"]
    assert an == bn, sorted(set(an) ^ set(bn))
    for u in range(len(RAGGED5)):
        for k in ("noise_z", "durations", "z_p", "z", "audio"):
            assert np.array_equal(a[u][k], b[u][k]), (u, k)


@pytest.mark.parametrize("lens,seed,wanted", [([900, 40], 14, {"attn_long_kernel<96>", "conv1x1_kernel<1>", "lngemm_kernel<6>"}),
                                              ([600], 36, {"attno_kernel<96>", "lngemm4_kernel"})])
def test_long_utterances_take_the_engines_own_attention_forms(lens, seed, wanted):
    """attn_long_kernel<96> (900 ids beside 40) and attno_kernel<96> (600 ids) as the engine's own choice. Only stage E and
    stage D are checked on the long utterance -- x_enc, m_p, logs_p, logw and every duration: its flow and generator in f64
    cost minutes on a CPU and add nothing, the same generator forms being covered at small shapes. The short neighbour, padded
    to 900 columns in every front-half launch, gets every stage for that reason. (PIPER_HIP_SPEC=0: module docstring.)"""
    _, names, _ = _case("medium", lens, seed, "PIPER_HIP_SPEC=0", {"PIPER_HIP_SPEC": 0}, stages={0: "ED"})
    U.require(names, wanted | {"duration_kernel", "regulate_kernel"}, lens)
    _gone(names, {"attn4_kernel<"}, lens)


def test_split_matrix_modes_on_a_ragged_batch():
    """Medium, RAGGED5, f32 / bf16x6 / f16x3 / bf16x3 on fresh engines (the same run counter, so the same prior noise): on every
    utterance all in front of the flow is the f32 run's bit for bit; z and audio meet truth_gates relative to the f32 run's
    error; the split kernels are named."""
    runs = {}
    for m in ("f32", "bf16x6", "f16x3", "bf16x3"):
        eng = U.engine_for("medium", {"PIPER_HIP_MATRIX": m}, fresh=True)
        try:
            runs[m] = _case("medium", RAGGED5, SEED5, "default", mode=m, eng=eng,
                            gated=U.STAGES if m == "f32" else ("x_enc", "m_p", "logs_p", "logw"))
        finally:
            eng.close()
        if m != "f32":
            assert any(f"split_kernel<{U.SM[m]}," in n for n in runs[m][1]), (m, sorted(runs[m][1]))
    f32, _, ffig = runs["f32"]
    for m, (got, _, fig) in runs.items():
        for u in range(len(RAGGED5)):
            for k in ("noise_z", "x_enc", "stats", "logw", "durations", "z_p"):
                assert np.array_equal(got[u][k], f32[u][k]), (m, u, k)
            for s in ("z", "audio"):
                err = {"torch": fig[u][s]["e_ref"], "fl": fig[u][s]["fl"], "f32": ffig[u][s]["e_hip"], m: fig[u][s]["e_hip"]}
                print(f"[{TARGET} medium {RAGGED5} default {m} utt {u}] {s}: {err}")
                assert U.truth_gates(err, m, "gauss"), (m, u, s, err)
