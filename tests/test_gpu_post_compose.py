"""A coupling layer's post composed into its WN skip convs (PIPER_HIP_WN_COMPOSE=1, engine_pack.cpp pack_post4) on an MI355X
(run with -m gpu), against the route with only pre composed (PIPER_HIP_WN_COMPOSE=2), both on fresh engines -- the same run
counter, so the same prior noise and the same z_p.

Medium at 3, 37 and 128 ids and the ragged call of 7 and 128 ids, high at 64 ids: each knob value meets every check of
tests/one_utterance_truth_case.py (z and audio: the f64 truth gates, K = 8; measured ratios in profiles/post_compose.md);
durations, frame counts, prior noise, z_p, the encoder's outputs and logw are equal bit for bit; the launch maps are equal
kernel name by kernel name (the composition changes what the launches compute, not which launches run); z differs, so the
composed route really ran. Post alone (PIPER_HIP_WN_COMPOSE=4, where the chain launch still computes the next layer's pre
behind the subtraction) against the route without compositions, medium at 37 ids: the same checks.

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


def _run(vname, ids, nw, env, route):
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
    U.check_call("gpu", vname, ids, U.SCALES, None, nw, got, route)
    return got, names


def _inputs(vname, lens):
    cfg, _ = U.voice(vname)
    if len(lens) == 1:
        return U.one_inputs(cfg, lens[0], 3, 100 + lens[0])
    ids, nw, _ = U.batch_inputs(cfg, lens, 31)
    return ids, nw


@pytest.mark.parametrize("vname,lens", [("medium", [3]), ("medium", [37]), ("medium", [128]), ("medium", [7, 128]), ("high", [64])])
def test_post_composed_against_pre_alone(vname, lens):
    cfg, _ = U.voice(vname)
    ids, nw = _inputs(vname, lens)
    a, an = _run(vname, ids, nw, {"PIPER_HIP_WN_COMPOSE": 2}, "WN_COMPOSE=2")
    b, bn = _run(vname, ids, nw, {"PIPER_HIP_WN_COMPOSE": 1}, "WN_COMPOSE=1")
    for u in range(len(ids)):
        assert a[u]["frames"] == b[u]["frames"]
        for k in ("durations", "noise_z", "z_p", "x_enc", "stats", "logw"):
            assert np.array_equal(a[u][k], b[u][k]), (u, k)
        assert not np.array_equal(a[u]["z"], b[u]["z"]), (u, "the composed route gave the bits of the route without it")
    assert an == bn, (an, bn)
    assert bn["colchain4_kernel<true>"] == cfg.flow_n and bn["gate4pre_kernel"] == cfg.flow_n, bn


def test_post_alone_against_the_plain_route():
    cfg, _ = U.voice("medium")
    ids, nw = _inputs("medium", [37])
    a, an = _run("medium", ids, nw, {"PIPER_HIP_WN_COMPOSE": 0}, "WN_COMPOSE=0")
    b, bn = _run("medium", ids, nw, {"PIPER_HIP_WN_COMPOSE": 4}, "WN_COMPOSE=4")
    assert a[0]["frames"] == b[0]["frames"]
    for k in ("durations", "noise_z", "z_p", "x_enc", "stats", "logw"):
        assert np.array_equal(a[0][k], b[0][k]), k
    assert not np.array_equal(a[0]["z"], b[0]["z"]), "the composed route gave the plain route's bits"
    assert an == bn and "gate4pre_kernel" not in bn and bn["colchain4_kernel<true>"] == cfg.flow_n, (an, bn)
