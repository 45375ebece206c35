"""The one-utterance path stage by stage against f64 truths on an MI355X (run with -m gpu): the text encoder, the duration
predictor with its spline, the durations' ceil, the length regulator, the flow and the generator, each from the engine's own
input to that stage (tests/one_utterance_truth_case.py has the checks and the gates; profiles/one_utterance_truth.md the
measured ratios and the reason for every gate).

The compared call is the repeated call of a warm engine -- the whole utterance as one graph, regulate_kernel computing the
durations -- with the engine's own prior noise; the kernel names are those of a profiled repeat that must reproduce its
durations and z_p bit for bit. Duration-noise seeds keep the oracle's own f64 durations at least 1e-4 (relative) from an
integer: 0.041 (3 ids), 0.030 (5), 2.5e-3 (64), 1.3e-4 (128), 1.7e-3 (129), 2.0e-3 (37), 6.8e-3 (40 at length_scale 1.3),
0.019 and 1.2e-4 (7 and 128 in one call), 2.5e-3 (high, 64), 1.7e-3 (x-low, 64), 4.2e-3 (tiny-ms, 33, speaker 2).

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import numpy as np
import pytest

import one_utterance_truth_case as U

pytestmark = pytest.mark.gpu

# the 192-channel one-utterance kernels of the default policy (attention: <96,false> up to 128 ids, <96,true> above)
FRONT4 = {"colchain4_kernel<false>", "lngemm4_kernel", "ffn_kernel", "dds_layer4_kernel", "regulate_kernel"}
FLOW4 = {"gate4_kernel", "colchain4_kernel<true>"}
GEN1 = {"conv_splitk_kernel<", "conv_splitk_group_kernel<", "pcm16_kernel"}
# (knob flipped, the policy it is flipped from, ids). The default policy sends the medium voice's WN gate conv to gate4_kernel at
# every length, so the two knobs that shape the split-K gate conv are flipped from the policies that reach it.
ROUTES = [(k, "", T) for k in (
    "PIPER_HIP_COL4=0", "PIPER_HIP_ATTN4=0", "PIPER_HIP_ATTNO=0", "PIPER_HIP_FFN=0", "PIPER_HIP_STACK_PRE=0", "PIPER_HIP_CHAIN_RS=0",
    "PIPER_HIP_FUSE_DP=0", "PIPER_HIP_GATE4=0", "PIPER_HIP_SPLITK16=0", "PIPER_HIP_SPLITK_MAX=0", "PIPER_HIP_GROUP_MRF=0",
    "PIPER_HIP_MRF_TAIL=0", "PIPER_HIP_SPEC=0", "PIPER_HIP_NO_GRAPH=1") for T in (37, 128)] + [
    ("PIPER_HIP_GATE_HALF=0", "PIPER_HIP_GATE4=0", 37),          # (128 ids: whole groups either way)
    ("PIPER_HIP_WIDE_SPLITK=0", "PIPER_HIP_GATE4=0,PIPER_HIP_SPLITK16=0", 37),
    ("PIPER_HIP_WIDE_SPLITK=0", "PIPER_HIP_GATE4=0,PIPER_HIP_SPLITK16=0", 128)]
GRAPH = {"PIPER_HIP_SPEC=0": "two", "PIPER_HIP_NO_GRAPH=1": "none"}          # knobs that select no kernel: how the call is issued
# knob -> (kernels that must appear, kernels that must be gone) against the policy it is flipped from; a name, or a prefix
SELECTS = {
    "PIPER_HIP_COL4=0": ({"attn_kernel<96>", "colchain_kernel<6>", "lngemm_kernel<6>", "dds_layer16_kernel<6>"},
                         {"attn4_kernel<", "colchain4_kernel<", "lngemm4_kernel", "dds_layer4_kernel", "ffn_kernel"}),
    "PIPER_HIP_ATTN4=0": ({"attno_kernel<96>"}, {"attn4_kernel<"}),
    "PIPER_HIP_ATTNO=0": ({"attn_kernel<96>"}, {"attn4_kernel<"}),
    "PIPER_HIP_FFN=0": (set(), {"ffn_kernel"}),
    "PIPER_HIP_CHAIN_RS=0": (set(), {"colchain4_kernel<true>"}),
    "PIPER_HIP_FUSE_DP=0": ({"cf_pre_kernel", "scale_kernel", "spline_inverse_kernel"}, set()),
    "PIPER_HIP_GATE4=0": ({"conv_splitk16_kernel<true,"}, {"gate4_kernel"}),
    "PIPER_HIP_SPLITK16=0": (set(), {"conv_splitk16_kernel<"}),
    "PIPER_HIP_SPLITK_MAX=0": ({"conv_mfma_kernel<2,2,2,1,16,true,64>", "conv_mfma_group_kernel<", "mrf_sum_kernel"},
                               {"conv_splitk_kernel<", "conv_splitk16_kernel<", "conv_splitk_group_kernel<", "gate4_kernel"}),
    "PIPER_HIP_GROUP_MRF=0": ({"conv_mfma_kernel<2,2,1,1,16,false,128>"}, {"conv_splitk_group_kernel<", "conv_splitk_sum_kernel<"}),
    "PIPER_HIP_MRF_TAIL=0": ({"conv_post_kernel"}, set()),
    "PIPER_HIP_GATE_HALF=0": ({"conv_splitk16_kernel<true,12,2,4>"}, {"conv_splitk16_kernel<true,6,5,2>"}),
    "PIPER_HIP_WIDE_SPLITK=0": ({"conv_splitk_kernel<2,true,8,3>"}, {"conv_splitk_kernel<2,true,12,2>"}),
}

_POLICY = {}         # (policy, T) -> (tensors, names, figures) on the medium voice


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()
    U.print_table("gpu")          # (with -s: the figures kept in profiles/one_utterance_truth.md)


def _case(vname, ids, nw, route, env=None, scales=U.SCALES, sids=None, graph="spec", mode="f32", eng=None, gated=U.STAGES):
    from piper_amd.engine import EngineError
    try:
        e = eng or U.engine_for(vname, env)
        got, names = U.run(e, ids, scales, sids, nw, graph=graph)
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {vname} {route}: {ex}", returncode=3)
    print(f"[gpu {vname} {[len(s) for s in ids]} {route} {mode}] kernels: {sorted(names)}")
    figs = U.check_call("gpu", vname, ids, scales, sids, nw, got, route, mode, gated=gated)
    return got, names, figs


def _medium(T, policy=""):
    """The medium voice at T ids under `policy` ("KNOB=v,KNOB=v", "" = the default), run once per module."""
    if (policy, T) not in _POLICY:
        cfg, _ = U.voice("medium")
        ids, nw = U.one_inputs(cfg, T, 3, 100 + T)
        env = dict(kv.split("=") for kv in policy.split(",") if kv)
        graph = ([GRAPH[kv] for kv in policy.split(",") if kv in GRAPH] + ["spec"])[0]
        _POLICY[policy, T] = _case("medium", ids, nw, policy or "default", env, graph=graph)
    return _POLICY[policy, T]


@pytest.mark.parametrize("T", [3, 5, 64, 128, 129])
def test_default_policy_medium(T):
    """3 ids: a single partial 4-column tile; 5: one full tile and one id; 64 and 128: the id-bucket edges, 128 the headline
    shape itself; 129: attn4_kernel<96,true>. (The half-group gate form needs PIPER_HIP_GATE4=0: ROUTES.)"""
    _, names, _ = _medium(T)
    U.require(names, FRONT4 | FLOW4 | GEN1 | {"attn4_kernel<96,true>" if T > 128 else "attn4_kernel<96,false>"}, T)


def test_two_ragged_utterances_in_one_call():
    """7 and 128 ids: ragged lengths, the utterance index on blockIdx.y / blockIdx.z."""
    cfg, _ = U.voice("medium")
    ids, nw, _ = U.batch_inputs(cfg, [7, 128], 31)
    _, names, _ = _case("medium", ids, nw, "default")
    U.require(names, FRONT4 | FLOW4 | {"attn4_kernel<96,false>", "conv_splitk_kernel<", "conv_mfma_kernel<", "mrf_kernel<", "pcm16_kernel"},
              "7 + 128")


# what each of the other voices is there for: the 4-column front and flow with the ResBlock1 generator's grouped split-K and
# tiled launches (high), the 96-channel forms (x-low), the conditioning launch with the generic-width forms (tiny-ms)
OTHERS = {
    "high": FRONT4 | FLOW4 | {"attn4_kernel<96,false>", "conv_splitk_group_kernel<4,2,128>", "conv_splitk_group_kernel<4,2,64>",
                              "conv_mfma_group_kernel<", "mrf_kernel<", "mrf_sum_kernel", "pcm16_kernel"},
    "x-low": {"attn_kernel<48>", "ln_kernel", "dds_layer16_kernel<3>", "conv_splitk_kernel<2,true,", "conv_splitk_kernel<1,false,",
              "conv_splitk16_kernel<false,", "conv_splitk_group_kernel<", "conv_mfma_kernel<", "mrf_kernel<", "regulate_kernel", "pcm16_kernel"},
    "tiny-ms": {"cond_kernel", "attn_kernel<0>", "ln_kernel", "dds_layer16_kernel<8>", "conv_splitk_kernel<2,true,", "conv_splitk_kernel<1,false,",
                "conv_mfma_kernel<", "mrf_kernel<", "regulate_kernel", "pcm16_kernel"},
    "medium": FRONT4 | FLOW4 | GEN1 | {"attn4_kernel<96,false>"},
}


@pytest.mark.parametrize("vname,T,index,seed,scales,sid", [
    ("high", 64, 3, 164, U.SCALES, None), ("x-low", 64, 3, 164, U.SCALES, None), ("tiny-ms", 33, 2, 53, U.SCALES, 2),
    ("medium", 40, 3, 140, (0.667, 1.3, 0.8), None)])
def test_other_voices_and_scales(vname, T, index, seed, scales, sid):
    """high (ResBlock1 generator), x-low (96 channels: none of the 4-column kernels), tiny-ms with speaker 2 (dp.cond and the WN
    conditioning), medium at length_scale 1.3."""
    cfg, _ = U.voice(vname)
    ids, nw = U.one_inputs(cfg, T, index, seed)
    _, names, _ = _case(vname, ids, nw, "default", scales=scales, sids=None if sid is None else [sid])
    U.require(names, OTHERS[vname], vname)


@pytest.mark.parametrize("knob,base,T", ROUTES)
def test_routes_compute_the_same_function(knob, base, T):
    """One knob flipped at 37 ids (one column past a 4-, a 12- and a 16-column tile) and at 128: the same function, the same
    gates. A knob that selects kernels must launch the kernels of SELECTS and none of those it replaces (PIPER_HIP_STACK_PRE=0:
    the same kernels in one launch more); the two that only change how the call is issued must leave names and launch
    counts alone."""
    _, ref, _ = _medium(T, base)
    _, names, _ = _medium(T, ",".join(x for x in (base, knob) if x))
    if knob in GRAPH:
        assert names == ref, (knob, sorted(set(names) ^ set(ref)))
    elif knob == "PIPER_HIP_STACK_PRE=0":
        assert set(names) == set(ref) and sum(names.values()) == sum(ref.values()) + 1, (names, ref)
        assert names["colchain4_kernel<false>"] == ref["colchain4_kernel<false>"] + 1, (names, ref)          # dp.pre on its own
    else:
        appear, gone = SELECTS[knob]
        U.require(names, appear, knob)
        assert set(names) != set(ref) and not [n for n in appear if n in ref], (knob, T, sorted(ref))
        for n in gone:
            U.require(ref, {n}, (knob, "flipped from a policy that does not launch it"))
            assert not [x for x in names if x == n or (n[-1] in "<," and x.startswith(n))], (knob, n, sorted(names))


@pytest.mark.parametrize("T", [37, 128])
def test_upconv_store_forms_are_bit_identical(T):
    """PIPER_HIP_CONVT_VEC=0 selects no kernel: the polyphase up-convs store their tile one 4-byte sample at a time instead
    of in 16- / 8-byte pieces (at 37 ids with a ragged last tile). Both forms on fresh engines -- the same run counter, so
    the same prior noise: every gate met by each, the same {kernel: launches} map, and z and the audio equal bit for bit,
    which they can only be if the other form wrote every sample."""
    cfg, _ = U.voice("medium")
    ids, nw = U.one_inputs(cfg, T, 3, 100 + T)
    runs = {}
    for route, env in (("default", {}), ("PIPER_HIP_CONVT_VEC=0", {"PIPER_HIP_CONVT_VEC": 0})):
        eng = U.engine_for("medium", env, fresh=True)
        try:
            runs[route] = _case("medium", ids, nw, route, eng=eng)
        finally:
            eng.close()
    (a, an, _), (b, bn, _) = runs["default"], runs["PIPER_HIP_CONVT_VEC=0"]
    assert an == bn, sorted(set(an) ^ set(bn))
    U.require(bn, FRONT4 | FLOW4 | GEN1, T)
    for k in ("noise_z", "durations", "z_p", "z", "audio"):
        assert np.array_equal(a[0][k], b[0][k]), (T, k)


def test_matrix_modes_on_the_one_utterance_path():
    """Medium, 128 ids, f32 / bf16x6 / f16x3 / bf16x3 on fresh engines (the same run counter, so the same prior noise): all
    in front of the flow is the f32 run's bit for bit; z and audio meet truth_gates relative to the f32 run's error."""
    cfg, _ = U.voice("medium")
    ids, nw = U.one_inputs(cfg, 128, 3, 100 + 128)
    runs = {}
    for m in ("f32", "bf16x6", "f16x3", "bf16x3"):
        eng = U.engine_for("medium", {"PIPER_HIP_MATRIX": m}, fresh=True)
        try:
            runs[m] = _case("medium", ids, nw, "default", mode=m, eng=eng,
                            gated=U.STAGES if m == "f32" else ("x_enc", "m_p", "logs_p", "logw"))
        finally:
            eng.close()
        if m != "f32":
            assert any(f"split_kernel<{U.SM[m]}," in n for n in runs[m][1]), (m, sorted(runs[m][1]))
    f32, _, ffig = runs["f32"]
    for m, (got, _, fig) in runs.items():
        for k in ("noise_z", "x_enc", "stats", "logw", "durations", "z_p"):
            assert np.array_equal(got[0][k], f32[0][k]), (m, k)
        for s in ("z", "audio"):
            err = {"torch": fig[0][s]["e_ref"], "fl": fig[0][s]["fl"], "f32": ffig[0][s]["e_hip"], m: fig[0][s]["e_hip"]}
            print(f"[gpu medium [128] default {m}] {s}: {err}")
            assert U.truth_gates(err, m, "gauss"), (m, s, err)
