"""Per-utterance noise seeds (include/piper_hip.h: pe_seeds) on an MI355X (run with -m gpu): the law in every kernel that
draws and in every graph form, mixed batches, independence of the handle and of the position in the batch, the seed against
injected noise, the serving paths at nonzero noise scales (mixed coalescer, group, streams, pool), graphs and launches, and
the refusal. tests/seeds_case.py holds what this file shares with tests/test_seeds_emu.py; profiles/seeds.md the figures.

"Exact" is np.array_equal against debug_randn(site, 0, n, row=c) of a second handle under set_seed(S), plus rng_case.check
against the f64 truth under rng_case's device gate (DEVICE_FACTOR * reference_error()). Two runs fed identical noise are held
to seeds_case.PCM_LSB = 7 LSB of int16 against each other (2e-4 of full scale, the project's figure for one path against
the oracle, is 6.6 LSB).

Left out: the prior noise of a batch stream. pe_debug_tensor refuses noise_z while a batch stream is open (its buffer holds
the chunk windows) -- the omission of tests/test_gpu_rng.py -- so only the stream's duration noise is compared.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import threading

import numpy as np
import pytest

import one_utterance_truth_case as U
import rng_case as R
import seeds_case as S
from piper_amd import weights as W

pytestmark = pytest.mark.gpu
POOL_TOL = 2e-4          # tests/test_gpu_stream_pool.py: a slot's concatenated chunks against the whole call (TIGHT_AUDIO_TOL)


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    U.close_engines()


def _gate():
    return R.DEVICE_FACTOR * R.reference_error()


def _guarded(fn, what):
    from piper_amd.engine import EngineError
    try:
        return fn()
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {what}: {ex}", returncode=3)


def _oracle():
    """The handle whose debug_randn gives the expected draws: the engines under test keep their own seed and counter."""
    return U.engine_for("tiny")


def _fresh(vname, env=None, seed=None):
    eng = _guarded(lambda: U.engine_for(vname, env, fresh=True), f"engine {vname}")
    if seed is not None:
        eng.set_seed(seed)
    return eng


def _seeded_calls(vname, lens, what, env=None, graph=None, scales=S.SCALES, runs=5, engine_seed=77):
    """Calls 1 .. runs of a fresh engine, every utterance seeded, the seeds moving from call to call (the second, third and
    last call share theirs: same frames, same graph keys) -- each checked exact at both sites -- then one more under the
    level-2 profile. `graph` as in rng_case.product_calls. Returns ({kernel: launches} of the profiled call, its frames)."""
    cfg, _ = U.voice(vname)
    ids = S.ids_of(cfg, lens)
    eng = _fresh(vname, env, engine_seed)
    oracle = _oracle()
    B = len(lens)

    def go():
        replays = 0
        for call in range(1, runs + 1):
            seeds = S.seeds_for(B, 1 if call in (2, 3, runs) else call)
            s0, g0 = eng.speculation_stats, eng.graph_stats
            eng.synthesize_batch(ids, scales, seeds=seeds)
            s1, g1 = eng.speculation_stats, eng.graph_stats
            print(f"[{what}] call {call}: speculation {s0} -> {s1} graphs {g0} -> {g1}")
            if graph is not None and call >= 2:
                if graph == "spec":
                    assert s1[0] == s0[0] + 1 and s1[1] == s0[1], (what, call, "not the one whole-utterance graph", s0, s1)
                else:
                    assert s1 == s0, (what, call, graph, s0, s1)
                assert (g1[0] == 0) == (graph == "none"), (what, call, graph, g1)
            replays += call >= 2 and g1[0] > 0 and g1[1] == g0[1]
            assert eng.rng_calls == call
            S.check_noise(eng, oracle, cfg, seeds, lens, _gate(), f"{what} call {call}")
        assert graph in (None, "none") or replays >= 1, (what, "no call replayed a captured graph")
        seeds = S.seeds_for(B, 2)
        names = S.profiled_names(eng, lambda: eng.synthesize_batch(ids, scales, seeds=seeds))
        frames = S.check_noise(eng, oracle, cfg, seeds, lens, _gate(), f"{what} profiled")
        print(f"[{what}] frames {frames} draw kernels: { {k: v for k, v in names.items() if k in R.DRAW_KERNELS} }")
        return names, frames
    try:
        return _guarded(go, what)
    finally:
        eng.close()


# ---- 1. the law, in every drawing kernel
def test_law_ragged_batch():
    """3, 5, 40 and 129 ids: a randn_kernel launch, the key per workgroup (row / 2); ragged rows."""
    names, frames = _seeded_calls("tiny", [3, 5, 40, 129], "tiny ragged", runs=2)
    assert "randn_kernel" in names and "regulate_kernel" in names, sorted(names)


@pytest.mark.parametrize("T, drawn_by", [(128, "embed_kernel"), (129, "randn_kernel")])
def test_law_both_sides_of_the_embed_seam(T, drawn_by):
    """Four utterances of 128 ids: 256 Philox blocks, embed_kernel picks the key per block; 129 ids: a randn_kernel launch."""
    names, _ = _seeded_calls("tiny", [T] * 4, f"tiny 4 x {T}", runs=2)
    assert ("randn_kernel" in names) == (drawn_by == "randn_kernel") and "embed_kernel" in names and "regulate_kernel" in names, sorted(names)


@pytest.mark.parametrize("env, graph", [({}, "spec"), ({"PIPER_HIP_SPEC": 0}, "two"), ({"PIPER_HIP_NO_GRAPH": 1}, "none")])
def test_law_medium_one_utterance(env, graph):
    """37 ids in every graph form: embed_kernel draws the duration noise, regulate_kernel the prior noise (with `fold` in the
    one-graph form); new seed values replay the captured graphs."""
    names, _ = _seeded_calls("medium", [37], f"medium 37 {graph}", env, graph)
    assert "randn_kernel" not in names and "embed_kernel" in names and "regulate_kernel" in names, sorted(names)


def test_law_xlow_voice():
    """inter = 96 rows at site 1, 33 ids."""
    cfg, _ = U.voice("x-low")
    assert cfg.inter == 96
    names, _ = _seeded_calls("x-low", [33], "x-low 33", graph="spec", runs=3)
    assert "randn_kernel" not in names and "regulate_kernel" in names, sorted(names)


def test_law_more_than_1024_frames():
    """200 ids at length_scale 6: several workgroups of regulate_kernel along one channel."""
    _, frames = _seeded_calls("tiny", [200], "tiny 200 long", scales=(0.667, 6.0, 0.8), runs=2)
    assert frames[0] > 1024, frames


# ---- 2. mixed batch
@pytest.mark.parametrize("env", [{}, {"PIPER_HIP_IDS_ZC": 0}], ids=["zero-copy", "copied"])
def test_mixed_batch(env):
    """use = [1, 0, 1, 0] on 40, 23, 40 and 7 ids, the keys read from the pinned block or copied with it: rows 1 and 3 are the
    engine's own stream at (engine seed, call, row = b * channels + c), rows 0 and 2 their seeds'; the same ids under the same
    seed are the same utterance."""
    cfg, _ = U.voice("tiny")
    lens = [40, 23, 40, 7]
    ids = S.ids_of(cfg, lens)
    ids[2] = ids[0]
    seeds = [S.SEEDS[4], None, S.SEEDS[4], None]
    eng = _fresh("tiny", env, 999)

    def go():
        for call in (1, 2):
            r = eng.synthesize_batch(ids, S.SCALES, seeds=seeds)
            S.check_noise(eng, _oracle(), cfg, seeds, lens, _gate(), f"mixed call {call}", engine_seed=999, call=call)
            d = eng.durations()
            assert np.array_equal(eng.debug_tensor("noise_w", 0), eng.debug_tensor("noise_w", 2))
            assert np.array_equal(eng.debug_tensor("noise_z", 0), eng.debug_tensor("noise_z", 2))
            assert np.array_equal(d[:40], d[63:103]) and r.frames[0] == r.frames[2]
        eng.synthesize_batch(ids, S.SCALES)
        R.check_engine_noise(eng, cfg, 999, 3, lens, _gate(), "unseeded after seeded")
    try:
        _guarded(go, "mixed")
    finally:
        eng.close()


# ---- 3. independence of the handle
def test_independent_of_the_handle():
    """Engine seeds 1 and 999, the second handle with three unrelated calls behind it: the same seeded call of 37 and 90 ids
    gives the same audio, sample for sample. pe_run twice on one seeded upload: the same results, rng_calls grown by 2."""
    cfg, _ = U.voice("medium")
    ids = S.ids_of(cfg, [37, 90])
    seeds = S.seeds_for(2, 3)
    a, b = _fresh("medium", None, 1), _fresh("medium", None, 999)

    def go():
        b.synthesize_batch(S.ids_of(cfg, [50], first=3), S.SCALES)
        b.synthesize_batch(S.ids_of(cfg, [20, 61, 33], first=9), S.SCALES)
        b.synthesize_batch(S.ids_of(cfg, [37, 90], first=20), S.SCALES, seeds=[5, None])
        ra, rb = a.synthesize_batch(ids, S.SCALES, seeds=seeds), b.synthesize_batch(ids, S.SCALES, seeds=seeds)
        assert (a.rng_calls, b.rng_calls) == (1, 4)
        assert np.array_equal(ra.frames, rb.frames), (ra.frames, rb.frames)
        for u in range(2):
            da = float(np.max(np.abs(ra.audio[u] - rb.audio[u])))
            print(f"[handles] utterance {u}: frames {int(ra.frames[u])} max |audio a - audio b| {da:.3e}")
        for u in range(2):
            assert np.array_equal(ra.audio[u], rb.audio[u]) and np.array_equal(ra.pcm[u], rb.pcm[u]), u
        a.upload(ids, S.SCALES, seeds=seeds)
        n0 = a.rng_calls
        a.run()
        r1 = a.fetch()
        a.run()
        r2 = a.fetch()
        assert a.rng_calls == n0 + 2
        for u in range(2):
            assert np.array_equal(r1.audio[u], r2.audio[u]) and np.array_equal(r1.pcm[u], r2.pcm[u]), u
    try:
        _guarded(go, "handles")
    finally:
        a.close()
        b.close()


# ---- 4. independence of the position
def test_independent_of_the_position():
    """Four texts with four seeds, in the order given and reversed: noise exact, durations and frames equal, pcm within 7 LSB."""
    cfg, _ = U.voice("tiny")
    lens = [40, 23, 31, 7]
    ids = S.ids_of(cfg, lens)
    seeds = S.seeds_for(4, 1)
    eng = _fresh("tiny", None, 3)

    def go():
        fwd = eng.synthesize_batch(ids, S.SCALES, seeds=seeds)
        S.check_noise(eng, _oracle(), cfg, seeds, lens, _gate(), "position forward")
        d_fwd = np.split(eng.durations(), np.cumsum(lens)[:-1])
        rev = eng.synthesize_batch(ids[::-1], S.SCALES, seeds=seeds[::-1])
        S.check_noise(eng, _oracle(), cfg, seeds[::-1], lens[::-1], _gate(), "position reversed")
        d_rev = np.split(eng.durations(), np.cumsum(lens[::-1])[:-1])
        same = []
        for u in range(4):
            assert np.array_equal(d_fwd[u], d_rev[3 - u]) and fwd.frames[u] == rev.frames[3 - u], u
            same.append(S.pcm_close(fwd.pcm[u], rev.pcm[3 - u], f"position utt {u}"))
        print(f"[position] bit-equal pcm per utterance: {same}")
    try:
        _guarded(go, "position")
    finally:
        eng.close()


# ---- 5. / 6. seed against injection
def test_seed_against_injection_and_injection_wins_per_site():
    """The seeded call against the call fed debug_randn's arrays at both sites: durations and frames equal, pcm within 7 LSB.
    noise_w injected beside a seed: noise_w is the injected array, noise_z the seed's."""
    cfg, _ = U.voice("tiny")
    lens = [40]
    ids = S.ids_of(cfg, lens)
    seed = S.SEEDS[3]
    eng = _fresh("tiny", None, 5)
    oracle = _oracle()

    def go():
        base = eng.synthesize_batch(ids, S.SCALES, seeds=[seed])
        d0 = eng.durations()
        F = int(base.frames[0])
        inj_w = S.expected(oracle, seed, 0, 0, 0, 2, 40)[None]
        inj_z = S.expected(oracle, seed, 0, 1, 0, cfg.inter, F)[None]
        r = eng.synthesize_batch(ids, S.SCALES, noise_w=inj_w, noise_z=inj_z)
        assert np.array_equal(eng.durations(), d0) and np.array_equal(r.frames, base.frames)
        S.pcm_close(r.pcm[0], base.pcm[0], "seed against injection")
        nw = np.random.default_rng(3).standard_normal((1, 2, 40)).astype(np.float32)
        eng.synthesize_batch(ids, S.SCALES, noise_w=nw, seeds=[seed])
        assert np.array_equal(eng.debug_tensor("noise_w", 0), nw[0])
        S.check_noise(eng, oracle, cfg, [seed], lens, _gate(), "injected w", sites=(1,))
    try:
        _guarded(go, "injection")
    finally:
        eng.close()


# ---- 7. serving paths, at nonzero noise scales
def test_mixed_coalescer_under_noise():
    """Eight threads, six seeded and two not, as ONE engine call: each seeded request is its own seeded B = 1 call on the same
    engine afterwards -- frames equal, pcm within 7 LSB."""
    from piper_amd.group import Coalescer
    cfg, _ = U.voice("tiny")
    lens = [40, 23, 31, 17, 40, 9, 28, 35]
    ids = S.ids_of(cfg, lens)
    seeds = [S.SEEDS[0], S.SEEDS[1], None, S.SEEDS[2], S.SEEDS[3], None, S.SEEDS[4], 12345]
    eng = _fresh("tiny", None, 21)
    co = Coalescer(eng, max_batch=8, max_wait_us=2000000, mix_scales=True)
    out, errs = [None] * 8, []

    def work(i):
        try:
            out[i] = co.synthesize(ids[i], S.SCALES, seed=seeds[i])
        except Exception as ex:              # noqa: BLE001
            errs.append(ex)
    try:
        th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
        [t.start() for t in th]
        [t.join() for t in th]
        if errs:
            pytest.exit(f"HIP / engine error in the coalescer: {errs[0]}", returncode=3)
        assert co.stats == (1, 8)

        def after():
            for i in range(8):
                if seeds[i] is None:
                    continue
                one = eng.synthesize(ids[i], S.SCALES, seed=seeds[i])
                pcm, frames, _, bs = out[i]
                assert bs == 8 and frames == int(one.frames[0]), (i, frames, one.frames)
                S.pcm_close(pcm, one.pcm[0], f"coalescer request {i}")
        _guarded(after, "coalescer")
    finally:
        co.close()
        eng.close()


def test_group_under_noise(monkeypatch):
    """EngineGroup [0, 0] with both members taking part: each member's utterances hold their seeds' noise, and the result is
    one engine's seeded call in the caller's order."""
    from piper_amd.group import EngineGroup
    cfg, w = U.voice("tiny")
    lens = [40, 23, 31, 7]
    ids = S.ids_of(cfg, lens)
    seeds = S.seeds_for(4, 2)
    monkeypatch.setenv("PIPER_HIP_GROUP_COALESCE", "0")
    monkeypatch.setenv("PIPER_HIP_DEBUG_KEEP", "1")
    grp = EngineGroup(W.pack_blob(cfg, w), [0, 0])
    eng = _fresh("tiny", None, 4)

    def go():
        r = grp.synthesize_batch(ids, S.SCALES, seeds=seeds)
        assign = grp.assignment(4)
        assert sorted(set(assign)) == [0, 1]
        for m in (0, 1):
            mine = [u for u in range(4) if assign[u] == m]
            S.check_noise(grp.engine(m), _oracle(), cfg, [seeds[u] for u in mine], [lens[u] for u in mine], _gate(), f"group member {m}")
        one = eng.synthesize_batch(ids, S.SCALES, seeds=seeds)
        assert list(r.frames) == list(one.frames)
        for u in range(4):
            S.pcm_close(r.pcm[u], one.pcm[u], f"group utt {u}")
    try:
        _guarded(go, "group")
    finally:
        grp.close()
        eng.close()


def test_streams_and_pool_under_noise():
    """A seeded one-utterance stream: both sites exact after the first chunk. A seeded batch stream: its duration noise
    (module docstring). A seeded newcomer of a pool with two residents in mid-stream: the durations of its seeded whole-
    utterance call, and its concatenated float chunks within the pool's figure of that call's audio."""
    cfg, _ = U.voice("tiny")
    lens = [40, 23, 31]
    ids = S.ids_of(cfg, lens)
    seeds = S.seeds_for(3, 0)
    eng = _fresh("tiny", None, 8)
    oracle = _oracle()

    def go():
        chunks = eng.stream(ids[0], S.SCALES, chunk_frames=16, seed=seeds[0])
        next(chunks)
        frames = S.check_noise(eng, oracle, cfg, seeds[:1], lens[:1], _gate(), "stream")
        assert frames[0] == eng.stream_frames
        for _ in chunks:
            pass
        chunks = eng.stream_batch(ids, S.SCALES, chunk_frames=16, seeds=[seeds[0], None, seeds[2]])
        next(chunks)
        S.check_noise(eng, oracle, cfg, [seeds[0], None, seeds[2]], lens, _gate(), "batch stream", sites=(0,), engine_seed=8, call=2)
        for _ in chunks:
            pass
        whole = eng.synthesize_batch(ids[:1], S.SCALES, seeds=seeds[:1])
        d = eng.durations()
        assert int(whole.frames[0]) == frames[0]
        with eng.stream_pool(3, 512) as pool:
            pool.join(ids[1:], S.SCALES)
            pool.next(16)
            slot = pool.join(ids[:1], S.SCALES, seeds=seeds[:1])[0]
            assert np.array_equal(eng.durations(), d)
            got = []
            while True:
                out = pool.next(16)
                if not out:
                    break
                if slot in out:
                    got.append(out[slot][0])
            a = np.concatenate(got)
            assert a.shape == whole.audio[0].shape
            err = float(np.max(np.abs(a - whole.audio[0])))
            print(f"[pool] seeded newcomer against its whole call: max |d| {err:.3e}")
            assert err < POOL_TOL, err
    try:
        _guarded(go, "streams")
    finally:
        eng.close()


# ---- 8. graphs and launches, and what a seed costs
def test_graphs_launches_and_time():
    """Ten seeded calls of 37 ids with ten seeds: the captures stop after the first calls (the seeds are data), and a seeded
    call takes the launches of the unseeded call on the same engine. Printed: the median infer_seconds of 300 seeded and 300
    unseeded calls (profiles/seeds.md; no gate)."""
    cfg, _ = U.voice("medium")
    ids = S.ids_of(cfg, [37])
    eng = _fresh("medium", None, 6)

    def go():
        caps = []
        for k in range(10):
            eng.synthesize_batch(ids, S.SCALES, seeds=[1000 + 7919 * k])
            caps.append(eng.graph_stats[1])
            launches = eng.run_launches
        print(f"[graphs] captures after each of ten seeded calls: {caps}; launches of the last {launches}")
        assert caps[-1] == caps[4], caps
        for _ in range(3):
            eng.synthesize_batch(ids, S.SCALES)
        plain_launches = eng.run_launches
        eng.synthesize_batch(ids, S.SCALES, seeds=[42])
        assert eng.run_launches == plain_launches, (eng.run_launches, plain_launches)
        # (a new seed per call, as the unseeded calls move on by their counter: both kinds walk through the frame counts of
        # the text, and with them through the frame buckets, alike)
        t = {}
        for kind in ("unseeded", "seeded", "unseeded again", "seeded again"):
            sd = kind.startswith("seeded")
            t[kind] = float(np.median([eng.synthesize_batch(ids, S.SCALES, seeds=[k] if sd else None).infer_seconds for k in range(300)]))
        print("[time] median infer_seconds of 300 medium 37-id calls: " + ", ".join(f"{k} {v * 1e6:.1f} us" for k, v in t.items()))
    try:
        _guarded(go, "graphs")
    finally:
        eng.close()


# ---- 9. refusals
def test_seeds_without_a_seed_array_are_refused():
    """A pe_seeds with a NULL seed is refused with a message before anything changes: the next unseeded call is the engine's
    own stream at the next counter."""
    import ctypes as C
    from piper_amd import _lib as L
    cfg, _ = U.voice("tiny")
    lens = [23]
    ids = S.ids_of(cfg, lens)
    eng = _fresh("tiny", None, 77)
    lib = L.get_lib()
    try:
        _guarded(lambda: eng.synthesize_batch(ids, S.SCALES), "refusal")
        flat, offs = eng._pack(ids)
        sc = np.ascontiguousarray(np.tile(np.asarray(S.SCALES, np.float32), (1, 1)))
        bad, res = L.PeSeeds(), L.PeResult()
        i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
        args = (eng._h, flat.ctypes.data_as(i64p), offs.ctypes.data_as(i64p), 1, sc.ctypes.data_as(f32p), None, None)
        assert lib.pe_synthesize_batch_seeded(*args, C.byref(res), None, C.byref(bad)) != 0
        assert b"seed" in lib.pe_last_error()
        assert eng.rng_calls == 1
        _guarded(lambda: eng.synthesize_batch(ids, S.SCALES), "refusal")
        R.check_engine_noise(eng, cfg, 77, 2, lens, _gate(), "after the refusal")
    finally:
        eng.close()
