"""Speaker blends and caller-supplied speaker vectors (include/piper_hip.h: pe_blend) on an MI355X (run with
-m gpu): speaker_blend_kernel and the blended call at the smallest shapes that can break them -- gin 16 (a quarter of a
wave) and gin 512 (eight workgroups per utterance), B = 1, 3 and 9, the zero-copy and the copied input path, the captured
graphs and one pool join. tests/speaker_blend_case.py holds what this file shares with tests/test_speaker_blend_emu.py.

Gates: against the oracle those of tests/test_gpu_parity.py (equal integer durations, int16 RMS <= 1e-3); the two
consequences bit for bit; the vector law under the bound of speaker_blend_case.

Any HIP error ends the session: nothing more is started on a device that has reported one."""
import numpy as np
import pytest

import one_utterance_truth_case as U
import speaker_blend_case as K
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu
RMS_TOL = 1e-3           # tests/test_gpu_parity.py
POOL_TOL = 2e-4          # tests/test_gpu_stream_pool.py: a slot's concatenated chunks against the whole call
VOICES = {"tiny-ms": {}, "tiny-ms-gin512": dict(gin=512, n_speakers=12)}
_MADE = {}


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for _, _, eng in _MADE.values():
        eng.close()
    _MADE.clear()


def _guarded(fn, what):
    try:
        return fn()
    except EngineError as ex:
        pytest.exit(f"HIP / engine error in {what}: {ex}", returncode=3)


def _voice(name, copied=False):
    """(cfg, weights, engine) of tiny-ms or its gin-512 / 12-speaker variant, weights seed 1234; one engine per voice and
    input path. `copied`: an engine that copies every call's input block to the device (PIPER_HIP_IDS_ZC=0), the path calls
    beyond 65 536 padded ids take by themselves."""
    if (name, copied) not in _MADE:
        cfg = W.preset("tiny-ms", **VOICES[name])
        w = W.synthetic_weights(cfg, 1234)
        from piper_amd import _lib as L
        with U.policy_env(L.get_lib(), {"PIPER_HIP_IDS_ZC": 0} if copied else {}):
            _MADE[name, copied] = (cfg, w, _guarded(lambda: Engine(blob=W.pack_blob(cfg, w), device=0), f"engine {name}"))
    return _MADE[name, copied]


def _spk9(E, seed=5):
    """Nine entries that walk through every kind: blends of 1, 2, 3 and 8 components (one with a repeated id, negative
    weights and weights above 1 among them), vectors, plain ids."""
    rng = np.random.default_rng(seed)
    n, gin = E.shape
    v = lambda: rng.standard_normal(gin).astype(np.float32) * np.float32(0.5)      # noqa: E731
    return [{1: 0.7, 3: 0.3}, 2, v(), [(0, 1.5), (1, -0.5), (0, 0.25)], {n - 1: 1.0}, None,
            [(int(s), float(a)) for s, a in zip(rng.integers(n, size=8), rng.uniform(-1, 1, size=8).astype(np.float32))], v(), 1]


# ---- 1. truth
@pytest.mark.parametrize("name", list(VOICES))
def test_truth_against_the_oracle(name):
    """speaker_blend_case's three blends with injected noise against the oracle on the one-row table of each g."""
    cfg, w, eng = _voice(name)
    ids = K.ids_of(cfg)
    nw, nz = K.noise(cfg, 3, max(K.LENS))
    t = K.truth(w, cfg, (name, 1234), ids, K.SCALES, nw, nz, K.SPEAKERS)
    K.check_margin(t, f"gpu truth {name}")
    r = _guarded(lambda: eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, speakers=K.SPEAKERS), "truth")
    d = np.split(eng.durations(), np.cumsum(K.LENS)[:-1])
    for b in range(3):
        rms = K.pcm_rms(r.pcm[b], t[b]["pcm"]) if r.pcm[b].shape == t[b]["pcm"].shape else float("inf")
        print(f"[gpu truth {name}] utterance {b}: durations equal {np.array_equal(d[b], t[b]['durations'])}, int16 rms {rms:.3e}")
    for b in range(3):
        assert np.array_equal(d[b], t[b]["durations"]), (b, d[b], t[b]["durations"])
        assert r.pcm[b].shape == t[b]["pcm"].shape and K.pcm_rms(r.pcm[b], t[b]["pcm"]) <= RMS_TOL, b
    for b in (0, 2):
        assert not np.array_equal(t[b]["durations"], t[b]["first"]), b


# ---- 2. bit for bit, 3. the vector law in a call
@pytest.mark.parametrize("path", ["copied", "zero-copy"])
@pytest.mark.parametrize("B", [1, 3, 9])
@pytest.mark.parametrize("name", list(VOICES))
def test_consequences_and_vectors(name, B, path):
    """Every utterance of a plain call with sids again as the unit blend {s: 1.0} or as the vector speaker_embedding(s), the
    kinds alternating: audio, PCM and durations np.array_equal. Then a call of B mixed entries: debug_tensor("g") against
    the law. "copied": injected noise on an engine whose input block is copied to the device; "zero-copy": seeds alone, the
    blend read in place from the pinned block."""
    cfg, w, eng = _voice(name, copied=path == "copied")
    E = K.table(w)
    lens = [7, 3, 12, 5, 9, 1, 4, 8, 2][:B]
    ids = K.ids_of(cfg, lens)
    nw, nz = K.noise(cfg, B, max(lens), seed=40 + B)
    extra = dict(noise_w=nw, noise_z=nz) if path == "copied" else dict(seeds=list(range(100, 100 + B)))
    sids = [(3 * b + 1) % cfg.n_speakers for b in range(B)]

    def go():
        plain = eng.synthesize_batch(ids, K.SCALES, sids=sids, **extra)
        d0 = eng.durations()
        for first in (0, 1, 2):
            kinds = [(first + b) % 3 for b in range(B)]
            speakers = [{s: 1.0} if k == 0 else eng.speaker_embedding(s) if k == 1 else s for s, k in zip(sids, kinds)]
            if all(k == 2 for k in kinds):
                continue
            r = eng.synthesize_batch(ids, K.SCALES, speakers=speakers, **extra)
            assert np.array_equal(eng.durations(), d0), (first, "durations")
            for u in range(B):
                assert np.array_equal(r.audio[u], plain.audio[u]) and np.array_equal(r.pcm[u], plain.pcm[u]), (first, u, kinds[u])
                assert np.array_equal(eng.debug_tensor("g", u)[0], E[sids[u]]), (first, u)
        mixed = _spk9(E)[:B]
        eng.synthesize_batch(ids, K.SCALES, speakers=mixed, **extra)
        worst = max(K.check_vector(eng.debug_tensor("g", u), E, sp, f"gpu g {name} B {B} utt {u}") for u, sp in enumerate(mixed))
        print(f"[gpu g {name} B {B} {path}] worst |g - g64| / bound {worst:.3f}")
        eng.synthesize_batch(ids, K.SCALES, sids=sids, **extra)
        for u in range(B):
            assert np.array_equal(eng.debug_tensor("g", u)[0], E[sids[u]]), u
    _guarded(go, f"consequences {name} {B} {path}")


def test_mixing_kernel_alone():
    """pe_debug_blend at gin 512 with 12 speakers: 64 utterances, counts cycling -1, 0, 1, 8, a repeated id in every 8-blend;
    and at gin 16 with every kind."""
    for name in VOICES:
        cfg, w, eng = _voice(name)
        E = K.table(w)
        assert eng.speaker_dim == cfg.gin
        for s in range(cfg.n_speakers):
            assert np.array_equal(eng.speaker_embedding(s), E[s])
        speakers = K.debug_cases(E)
        out = _guarded(lambda: eng.debug_blend(speakers), f"debug_blend {name}")
        assert out.shape == (64, cfg.gin)
        worst = max(K.check_vector(out[b], E, sp, f"gpu debug_blend {name} utt {b}") for b, sp in enumerate(speakers))
        print(f"[gpu debug_blend {name} 64 x 8 x {cfg.gin}] worst |g - g64| / bound {worst:.3f}")


def test_beyond_the_zero_copy_threshold():
    """513 utterances padded to 128 ids are 65 664 padded ids: the call copies its input block, blend area in front, by
    itself, at a batch capacity the engine grows to for it. Unit blends, table rows as vectors and plain ids, three in turn,
    are bit for bit the plain call; the vectors of the first, a middle and the last utterance are their table rows."""
    cfg, w, eng = _voice("tiny-ms")
    E = K.table(w)
    B = 513
    ids = [K.ids_of(cfg, (2,))[0]] * B
    sids = [(3 * b + 1) % cfg.n_speakers for b in range(B)]
    rows = [E[s] for s in sids]
    speakers = [{s: 1.0} if b % 3 == 0 else rows[b] if b % 3 == 1 else s for b, s in enumerate(sids)]
    zero = (0.0, 1.0, 0.0)

    def go():
        plain = eng.synthesize_batch(ids, zero, sids=sids)
        d0 = eng.durations()
        r = eng.synthesize_batch(ids, zero, speakers=speakers)
        assert np.array_equal(eng.durations(), d0)
        for u in (0, 1, 256, 511, 512):
            assert np.array_equal(eng.debug_tensor("g", u)[0], rows[u]), u
        bad = [u for u in range(B) if not (np.array_equal(r.audio[u], plain.audio[u]) and np.array_equal(r.pcm[u], plain.pcm[u]))]
        assert not bad, bad[:8]
        assert any(not np.array_equal(plain.audio[0], plain.audio[u]) for u in range(1, 4))       # (the speakers do differ)
    _guarded(go, "beyond the zero-copy threshold")


# ---- graphs
def test_blend_values_are_data_for_the_graphs():
    """Blended B = 1 calls with other weights, kinds and vectors replay the captured graphs -- pe_graph_stats captures stay --
    in the speculative one-graph form -- pe_speculation_stats runs grow by one per call, without a miss; the plain call's
    graphs live beside them, and a blended call takes at most one launch more than the plain one."""
    cfg, w, eng = _voice("tiny-ms")
    ids = K.ids_of(cfg, (33,))
    E = K.table(w)

    def go():
        # (one seed, and weights a step of 1e-4 apart: the frame count stays, so that nothing but the values changes)
        first, other = {1: 0.7, 3: 0.3}, {1: 0.6999, 3: 0.3001}
        vec = K.law32(E, first) * np.float32(1.0001)
        for _ in range(4):
            eng.synthesize_batch(ids, K.SCALES, seeds=[7], speakers=[first])
        blended_launches = eng.run_launches
        s0, g0 = eng.speculation_stats, eng.graph_stats
        r1 = eng.synthesize_batch(ids, K.SCALES, seeds=[7], speakers=[first])
        s1, g1 = eng.speculation_stats, eng.graph_stats
        r2 = eng.synthesize_batch(ids, K.SCALES, seeds=[7], speakers=[other])
        s2, g2 = eng.speculation_stats, eng.graph_stats
        K.check_vector(eng.debug_tensor("g", 0), E, other, "graph replay, other weights")
        r3 = eng.synthesize_batch(ids, K.SCALES, seeds=[7], speakers=[vec])
        s3, g3 = eng.speculation_stats, eng.graph_stats
        K.check_vector(eng.debug_tensor("g", 0), E, vec, "graph replay, a vector")
        print(f"[gpu graphs] speculation {s0} -> {s1} -> {s2} -> {s3}; graphs {g0} -> {g1} -> {g2} -> {g3}; launches {blended_launches}; "
              f"frames {int(r1.frames[0])} {int(r2.frames[0])} {int(r3.frames[0])}")
        assert g1[1] == g0[1] and g2[1] == g0[1] and g3[1] == g0[1], (g0, g1, g2, g3)
        assert s1[0] == s0[0] + 1 and s2[0] == s1[0] + 1 and s3[0] == s2[0] + 1, (s0, s1, s2, s3)
        assert not np.array_equal(r1.audio[0], r2.audio[0]) or r1.audio[0].shape != r2.audio[0].shape
        for _ in range(4):
            eng.synthesize_batch(ids, K.SCALES, seeds=[7], sids=[1])
        assert eng.run_launches + 1 >= blended_launches >= eng.run_launches, (eng.run_launches, blended_launches)
    _guarded(go, "graphs")


# ---- one pool join
def test_pool_join_with_a_blend():
    """A blended newcomer beside a plain resident in mid-stream: its concatenated chunks are its whole blended call's audio
    within the pool's figure; the slot, left and taken by a plain utterance, delivers that utterance's own audio."""
    cfg, w, eng = _voice("tiny-ms")
    ids = K.ids_of(cfg, (23, 31))
    sp = {0: 1.5, 1: -0.5}
    zero = (0.0, 1.0, 0.0)

    def drain(pool, slot):
        out = []
        while True:
            step = pool.next(16)
            if not step:
                return np.concatenate(out)
            if slot in step:
                out.append(step[slot][0])

    def go():
        whole = eng.synthesize_batch(ids[:1], zero, speakers=[sp])
        plain = eng.synthesize_batch(ids[:1], zero, sids=[3])
        with eng.stream_pool(2, 1024) as pool:
            pool.join(ids[1:], zero, sids=[2])
            pool.next(16)
            slot = pool.join(ids[:1], zero, speakers=[sp])[0]
            a = drain(pool, slot)
            assert a.shape == whole.audio[0].shape
            err = float(np.max(np.abs(a - whole.audio[0])))
            print(f"[gpu pool] blended newcomer against its whole call: max |d| {err:.3e}")
            assert err < POOL_TOL, err
            again = pool.join(ids[:1], zero, speakers=[sp])[0]
            pool.next(16)
            pool.leave(again)
            slot3 = pool.join(ids[:1], zero, sids=[3])[0]
            assert slot3 == again
            b = drain(pool, slot3)
            assert b.shape == plain.audio[0].shape
            err = float(np.max(np.abs(b - plain.audio[0])))
            print(f"[gpu pool] plain tenant after a blended one: max |d| {err:.3e}")
            assert err < POOL_TOL, err
    _guarded(go, "pool")


def test_refusal_leaves_the_engine_alone():
    """A refused blend names the utterance and the component, and the next call is served."""
    cfg, w, eng = _voice("tiny-ms")
    ids = K.ids_of(cfg, (5, 4))
    with pytest.raises(EngineError, match="utterance 1, blend component 1"):
        eng.synthesize_batch(ids, K.SCALES, speakers=[None, [(0, 1.0), (4, 1.0)]])
    r = _guarded(lambda: eng.synthesize_batch(ids, K.SCALES, speakers=[None, [(0, 1.0), (3, 1.0)]]), "after the refusal")
    assert all(int(f) > 0 for f in r.frames)
