"""PIPER_HIP_WN_COMPOSE on an MI355X (run with -m gpu): a coupling layer's pre composed into its first gate conv
(gate4pre_kernel, kernels/gate4.h) against the route without it, both on fresh engines -- the same run counter, so the same
prior noise and the same z_p.

Medium at 3, 37 and 128 ids and the ragged call of 7 and 128 ids, high at 64 ids: each knob value meets every check of
tests/one_utterance_truth_case.py (z and audio: the f64 truth gates, K = 8; measured ratios in profiles/wn_compose.md);
durations, frame counts, prior noise and z_p are equal. The composed route runs one colchain4_kernel<false> launch fewer (the
first coupling layer's pre: 74 launches against 75 for medium at 128 ids), four gate4pre_kernel launches in place of as
many of gate4_kernel, and still gate4_kernel and colchain4_kernel<true>. Under PIPER_HIP_GATE4=0 the knob changes nothing: the
same launches, z and audio equal bit for bit. Under PIPER_HIP_CHAIN_RS=0 pre is composed all the same (that knob must keep
costing exactly one launch per coupling layer, tests/test_emu_engine.py), with the bits of the default route.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import numpy as np
import pytest

import one_utterance_truth_case as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()
    U.print_table("gpu")


def _run(vname, ids, nw, env, route, check=True):
    from piper_amd.engine import EngineError
    eng = None
    try:
        eng = U.engine_for(vname, env, fresh=True)
        got, names = U.run(eng, ids, U.SCALES, None, nw)
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {vname} {route}: {ex}", returncode=3)
    finally:
        if eng is not None:
            eng.close()
    print(f"[gpu {vname} {[len(s) for s in ids]} {route}] launches {sum(names.values())} kernels: {sorted(names.items())}")
    if check:
        U.check_call("gpu", vname, ids, U.SCALES, None, nw, got, route)
    return got, names


def _inputs(vname, lens):
    cfg, _ = U.voice(vname)
    if len(lens) == 1:
        return U.one_inputs(cfg, lens[0], 3, 100 + lens[0])
    ids, nw, _ = U.batch_inputs(cfg, lens, 31)
    return ids, nw


@pytest.mark.parametrize("vname,lens", [("medium", [3]), ("medium", [37]), ("medium", [128]), ("medium", [7, 128]), ("high", [64])])
def test_composed_route_against_the_plain_one(vname, lens):
    cfg, _ = U.voice(vname)
    ids, nw = _inputs(vname, lens)
    a, an = _run(vname, ids, nw, {"PIPER_HIP_WN_COMPOSE": 0}, "WN_COMPOSE=0")
    b, bn = _run(vname, ids, nw, {"PIPER_HIP_WN_COMPOSE": 1}, "WN_COMPOSE=1")
    for u in range(len(ids)):
        assert a[u]["frames"] == b[u]["frames"]
        for k in ("durations", "noise_z", "z_p", "x_enc", "stats", "logw"):
            assert np.array_equal(a[u][k], b[u][k]), (u, k)
        assert not np.array_equal(a[u]["z"], b[u]["z"]), (u, "the composed route gave the plain route's bits")
    want = dict(an)
    want["colchain4_kernel<false>"] -= 1
    want["gate4_kernel"] -= cfg.flow_n
    want["gate4pre_kernel"] = cfg.flow_n
    assert "gate4pre_kernel" not in an and an["gate4_kernel"] == cfg.flow_n * cfg.wn_layers, an
    assert bn == want, (bn, want)
    assert bn["gate4_kernel"] > 0 and bn["colchain4_kernel<true>"] == cfg.flow_n, bn
    assert sum(bn.values()) == sum(an.values()) - 1
    if (vname, lens) == ("medium", [128]):          # the profiled repeat: the step's 75 / 74 launches and one that injects the prior noise
        assert (sum(an.values()), sum(bn.values())) == (76, 75), (sum(an.values()), sum(bn.values()))


def test_knob_changes_nothing_without_gate4_kernel():
    ids, nw = _inputs("medium", [37])
    a, an = _run("medium", ids, nw, {"PIPER_HIP_GATE4": 0, "PIPER_HIP_WN_COMPOSE": 0}, "GATE4=0,WN_COMPOSE=0", check=False)
    b, bn = _run("medium", ids, nw, {"PIPER_HIP_GATE4": 0, "PIPER_HIP_WN_COMPOSE": 1}, "GATE4=0,WN_COMPOSE=1", check=False)
    assert an == bn and "gate4pre_kernel" not in bn, (an, bn)
    for k in ("durations", "noise_z", "z_p", "z", "audio"):
        assert np.array_equal(a[0][k], b[0][k]), k


def test_composed_route_with_the_last_res_skip_conv_on_its_own():
    """PIPER_HIP_CHAIN_RS=0 only moves the last res/skip conv of a coupling layer into a launch of its own (no
    colchain4_kernel<true>): pre is composed all the same, so that knob still costs one launch per coupling layer."""
    cfg, _ = U.voice("medium")
    ids, nw = _inputs("medium", [37])
    a, an = _run("medium", ids, nw, {"PIPER_HIP_CHAIN_RS": 0, "PIPER_HIP_WN_COMPOSE": 0}, "CHAIN_RS=0,WN_COMPOSE=0", check=False)
    b, bn = _run("medium", ids, nw, {"PIPER_HIP_CHAIN_RS": 0, "PIPER_HIP_WN_COMPOSE": 1}, "CHAIN_RS=0,WN_COMPOSE=1")
    c, cn = _run("medium", ids, nw, {"PIPER_HIP_WN_COMPOSE": 1}, "WN_COMPOSE=1", check=False)
    assert "colchain4_kernel<true>" not in an and "colchain4_kernel<true>" not in bn, (an, bn)
    assert bn["gate4pre_kernel"] == cfg.flow_n and sum(bn.values()) == sum(an.values()) - 1 == sum(cn.values()) + cfg.flow_n, (an, bn, cn)
    for k in ("durations", "noise_z", "z_p"):
        assert np.array_equal(a[0][k], b[0][k]), k
    for k in ("z", "audio"):          # the same additions in the same order as with the conv in front of the chain
        assert np.array_equal(b[0][k], c[0][k]), k
