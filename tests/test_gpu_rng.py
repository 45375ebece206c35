"""The noise generator on an MI355X (run with -m gpu) against the reference of tests/rng_case.py: every draw of 2^22 per site
against the f64 truth, the stream law over windows whose counter, stream and seed words all cross 2^32, the engine's own
noise in the product path wherever it is drawn (embed_kernel, a randn_kernel launch, regulate_kernel -- folded into the
one-utterance graph or not), and the seeds of a group's members. profiles/rng_truth.md holds the measured figures.

Gates (rng_case): on every element |g - t| <= 2^-13 max(1, rad) -- a draw from other integers, another pair order or the
other trig function is O(1) off; the normalised error E = max |g - t| / rad of the device is at most 16 times that of the
f32 reference (numpy's log2 / sin / cos on the same integers), four bits for the hardware's v_log_f32 / v_sin_f32 /
v_cos_f32 against libm. Windows and product-path tensors of a few draws are held to 16 times the reference's E over 2^22
draws (rng_case.reference_error): the maximum over a handful of draws is no estimate of the reference's error.

Left out: the prior noise of a batch stream. pe_debug_tensor refuses noise_z while a batch stream is open (its buffer holds
the chunk windows), so only the stream's duration noise is compared.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import numpy as np
import pytest

import one_utterance_truth_case as U
import rng_case as R
from piper_amd import weights as W

pytestmark = pytest.mark.gpu
SEED = 2026
ROWS = []          # (site, class, n, E_dev, E_ref, e_dev): the table of profiles/rng_truth.md


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()
    if ROWS:
        print("\n| site | draws | n | E_dev | E_ref | ratio | e_dev |\n|---|---|---|---|---|---|---|")
        for site, name, n, Ed, Er, ed in ROWS:
            print(f"| {site} | {name} | {n} | {Ed:.3e} | {Er:.3e} | {Ed / max(Er, 1e-300):.2f} | {ed:.3e} |")


def _gate():
    return R.DEVICE_FACTOR * R.reference_error()


def _guarded(fn, what):
    from piper_amd.engine import EngineError
    try:
        return fn()
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {what}: {ex}", returncode=3)


def _ids(cfg, lens, first=70):
    return [W.synthetic_phoneme_ids(T, first + i, id_max=min(cfg.n_vocab - 1, 129)) for i, T in enumerate(lens)]


def _product(vname, lens, what, env=None, graph=None, scales=R.SCALES, seed=77):
    cfg, _ = U.voice(vname)
    eng = _guarded(lambda: U.engine_for(vname, env, fresh=True), what)
    try:
        return _guarded(lambda: R.product_calls(eng, cfg, seed, _ids(cfg, lens), _gate(), f"gpu {what}", scales=scales, graph=graph), what)
    finally:
        eng.close()


@pytest.mark.parametrize("site", [0, 1])
def test_every_draw_of_a_site(site):
    """2^22 draws (64 stream rows) of one debug_randn, every element against t; E and e overall and per class of edge draws,
    and the error split into the radius (log2, sqrt) and the angle (sin, cos) of each pair."""
    eng = U.engine_for("tiny")
    n = R.EDGE_N
    eng.set_seed(SEED)
    g = _guarded(lambda: eng.debug_randn(site, 1, n), "debug_randn")
    t, rad, g32 = R.truth(SEED, 1, site, 0, 0, n)
    E_ref, e_ref, _ = R.errors(g32, t, rad)
    E_dev, e_dev, _ = R.errors(g, t, rad)
    ROWS.append((site, "all", n, E_dev, E_ref, e_dev))
    print(f"[gpu site {site}] all {n} draws: E_dev {E_dev:.3e} E_ref {E_ref:.3e} ratio {E_dev / E_ref:.2f} e_dev {e_dev:.3e} e_ref {e_ref:.3e} "
          f"max |t| {float(np.max(np.abs(t))):.2f}")
    edges = R.edge_draws(SEED, 1, site)
    for line in R.describe_edges(SEED, 1, site, edges):
        print(f"[gpu site {site}] {line}")
    for name in R.EDGE_CLASSES:
        p = edges[name]
        Ed, ed, _ = R.errors(g[p], t[p], rad[p])
        Er, _, _ = R.errors(g32[p], t[p], rad[p])
        ROWS.append((site, name, p.size, Ed, Er, ed))
        print(f"[gpu site {site}] {name}: E_dev {Ed:.3e} E_ref {Er:.3e} ratio {Ed / max(Er, 1e-300):.2f} e_dev {ed:.3e}")
    # where the error comes from: each pair's radius and unit vector (a figure, not a gate)
    gc, gs = g[0::2].astype(np.float64), g[1::2].astype(np.float64)
    r_dev, r_t = np.hypot(gc, gs), rad[0::2]
    ok = r_t > 0
    unit = np.maximum(np.abs(gc[ok] / r_dev[ok] - t[0::2][ok] / r_t[ok]), np.abs(gs[ok] / r_dev[ok] - t[1::2][ok] / r_t[ok]))
    print(f"[gpu site {site}] radius: max |hypot(g) - rad| / rad {float(np.max(np.abs(r_dev[ok] - r_t[ok]) / r_t[ok])):.3e}; "
          f"angle: max |g / hypot(g) - (cos, sin)| {float(np.max(unit)):.3e}")
    R.check(g, t, rad, R.DEVICE_FACTOR * E_ref, f"[gpu site {site}]")


def test_stream_law():
    eng = U.engine_for("tiny")
    worst = _guarded(lambda: R.check_windows(eng, _gate(), "gpu"), "windows")
    print(f"stream law: {len(R.windows())} windows, worst E {worst:.3e} gate {_gate():.3e}")


@pytest.mark.parametrize("env, graph", [({}, "spec"), ({"PIPER_HIP_SPEC": 0}, "two"), ({"PIPER_HIP_NO_GRAPH": 1}, "none")])
def test_medium_one_utterance(env, graph):
    """37 ids: embed_kernel's draw ends one column into a block; the prior noise comes from regulate_kernel (with `fold` in
    the one-graph form). Calls 1 to 4, at least one of them a replayed graph, and a profiled fifth; no randn_kernel launch."""
    names, _ = _product("medium", [37], f"medium 37 {graph}", env, graph)
    assert "randn_kernel" not in names and "embed_kernel" in names and "regulate_kernel" in names, sorted(names)


@pytest.mark.parametrize("T, drawn_by", [(128, "embed_kernel"), (129, "randn_kernel")])
def test_both_sides_of_the_embed_seam(T, drawn_by):
    """Tiny voice, four utterances: 128 ids are 4 * 2 * 32 = 256 Philox blocks, the most embed_kernel draws itself; 129 ids
    (the id bucket of 160: 320 blocks) go to a randn_kernel launch. The same law on both sides."""
    names, _ = _product("tiny", [T] * 4, f"tiny 4 x {T}")
    assert ("randn_kernel" in names) == (drawn_by == "randn_kernel") and "embed_kernel" in names and "regulate_kernel" in names, sorted(names)


def test_ragged_batch():
    """3, 5, 40 and 129 ids: rows 2 b + c and inter b + c of utterances of unequal lengths; no padding column is compared."""
    names, frames = _product("tiny", [3, 5, 40, 129], "tiny ragged", seed=2 ** 32 + 1)
    assert "randn_kernel" in names and len(set(frames)) == 4, (sorted(names), frames)


def test_xlow_voice():
    """inter = 96 rows per utterance at site 1, 33 ids."""
    cfg, _ = U.voice("x-low")
    assert cfg.inter == 96
    names, _ = _product("x-low", [33], "x-low 33", graph="spec")
    assert "randn_kernel" not in names, sorted(names)


def test_more_than_1024_frames():
    """200 ids at length_scale 6: several workgroups of regulate_kernel along the frames of one channel."""
    _, frames = _product("tiny", [200], "tiny 200 long", scales=(0.667, 6.0, 0.8))
    assert frames[0] > 1024, frames


def test_streams_draw_the_same_law():
    """A one-utterance stream: after the first chunk noise_w / noise_z are the reference's at the stream's run counter. A
    batch stream: its duration noise (module docstring: its noise_z cannot be read)."""
    cfg, _ = U.voice("tiny")
    ids = _ids(cfg, [40, 23])
    eng = _guarded(lambda: U.engine_for("tiny", fresh=True), "stream")
    try:
        eng.set_seed(31)

        def go():
            for call in (1, 2):
                chunks = eng.stream(ids[0], R.SCALES, chunk_frames=16)
                next(chunks)
                frames = R.check_engine_noise(eng, cfg, 31, call, [40], _gate(), "gpu tiny stream")
                assert frames[0] == eng.stream_frames
                for _ in chunks:
                    pass
            chunks = eng.stream_batch(ids, R.SCALES, chunk_frames=16)
            next(chunks)
            R.check_engine_noise(eng, cfg, 31, 3, [40, 23], _gate(), "gpu tiny batch stream", sites=(0,))
            for _ in chunks:
                pass
        _guarded(go, "stream")
    finally:
        eng.close()


def test_group_members_draw_distinct_streams(monkeypatch):
    """A group nobody seeded: member i draws from the default seed + i, in every group created that way."""
    _guarded(lambda: R.check_group(None, monkeypatch, "tiny", _gate(), "gpu"), "group")
