"""The stream pool on the MI355X (run with -m gpu): pe_stream_pool_* through piper_amd.engine.Engine.stream_pool. Listeners
join a live batch stream, finish, have their slot reused and leave (the scenario of tests/stream_pool_case.py) on the inputs
and at the bounds of tests/test_gpu_stream_batch.py; the emulator counterpart, with poisoned workspaces, a multi-speaker
voice, the survival and the error cases, is tests/test_stream_pool_emu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from piper_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import stream_pool_case as P                             # noqa: E402
import test_gpu_stream_batch as G                        # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("preset", list(G.CASES))
def test_listeners_join_finish_reuse_and_leave(preset):
    """Every delivered chunk of every listener equals the one-utterance stream's chunk (2e-5), carries the int16 of its own
    floats bit for bit, and matches the oracle's chunked decode of the oracle's latent (2e-4 / 1e-3 RMS); every listener
    has the chunks it has alone, the one that hung up the ones it received."""
    worst = P.gpu_case(preset, G.CHUNK_TOL, G.TIGHT_AUDIO_TOL, G.RMS_TOL, G.SCALES)
    print(f"[{preset}] {worst}")
    assert worst["one"] < G.CHUNK_TOL and worst["oracle"] < G.TIGHT_AUDIO_TOL and worst["rms"] <= G.RMS_TOL, worst
    assert len(worst["left"]) == 1 and min(worst["chunks"]) >= 1


def test_split_matrix_mode_in_a_child_process():
    """The medium scenario under PIPER_HIP_MATRIX=f16x3 (read at engine creation; a process of its own, so that no other
    test's engine shares the setting): the pool's chunks against the one-utterance stream of the same mode and against the
    oracle, at the f32 gate like the other split-mode tests."""
    from piper_amd import _lib as L
    env = dict(os.environ, PIPER_HIP_MATRIX="f16x3")
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())]:
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_pool_case.py"), "--gpu", "medium"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    worst = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"\n[medium, f16x3] {worst}")
    assert worst["one"] < G.CHUNK_TOL and worst["oracle"] < G.TIGHT_AUDIO_TOL and worst["rms"] <= G.RMS_TOL, worst


def frame_bucket(frames):
    """Engine::frame_bucket below 1024 frames: steps of 64."""
    assert 1 <= frames <= 1024
    return -(-frames // 64) * 64


def other_text(eng, cfg, like, role):
    """Another text of `like`'s length -- ids and duration noise from other seeds -- whose frame count falls into the same
    frame bucket: the first of up to 60 candidates that does (the count is the engine's, from a plain call)."""
    T = like.ids.size
    for k in range(60):
        seed = 500 + 60 * role + k
        ids = W.synthetic_phoneme_ids(T, seed, id_max=min(cfg.n_vocab - 1, 129))
        nw = np.random.default_rng(seed).standard_normal((2, T)).astype(np.float32)
        frames = int(eng.synthesize(ids, like.scales, noise_w=nw).frames[0])
        if frame_bucket(frames) == frame_bucket(like.frames):
            assert not np.array_equal(ids, like.ids)
            return P.Listener("ids%d/%d" % (T, seed), ids, like.scales, None, nw, None)
    raise AssertionError("no text of %d ids in the frame bucket of %d frames among 60 candidates" % (T, like.frames))


def test_second_cycle_of_the_same_buckets_captures_nothing():
    """One captured graph per (slots, window bucket) serves every call, whoever sits in which slot; the joins replay the
    stage graphs of their (n, id bucket, frame bucket), and stream_adopt_kernel is a plain launch. After one full cycle of
    joins, chunks and leaves a second one with OTHER texts of the same buckets -- other ids and other duration noise of the
    same lengths, each in its predecessor's frame bucket, the listeners of the big join in another order, new prior noise --
    captures nothing."""
    from piper_amd.engine import Engine
    cfg = W.preset("medium")
    eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    # injected duration noise fixes the frame counts (and with them the buckets), the prior noise is the engine's: every
    # stage of a join is a captured graph
    t1, chunk, first = P.gpu_texts(cfg, "medium", G.SCALES, prior_noise=False)
    with eng.stream_pool(len(t1) - 1, 512) as pool:
        P.play(eng, t1, chunk, first, pool=pool)
        # (the candidates run as plain calls on the same handle, the pool open: their graphs are captured here, before
        # the count the second cycle is held to)
        t2 = [other_text(eng, cfg, x, i) for i, x in enumerate(t1)]
        cached1, captures1 = eng.graph_stats
        P.play(eng, t2, chunk, first, pool=pool, second_order=list(range(len(t2) - 2))[::-1])
        cached2, captures2 = eng.graph_stats
    print(f"\n[medium x {len(t1)}] frames {[x.frames for x in t1]} then {[x.frames for x in t2]}: graphs cached / captured "
          f"after the first cycle {cached1} / {captures1}, after the second {cached2} / {captures2}")
    assert [frame_bucket(x.frames) for x in t1] == [frame_bucket(x.frames) for x in t2]
    assert [x.frames for x in t1] != [x.frames for x in t2] and t1[0].slot != t2[0].slot
    assert all(len(x.chunks) >= 1 for x in t2)
    assert captures1 > 0 and captures2 == captures1 and cached2 == cached1
    eng.close()


def test_64_slots_joining_in_four_waves_equal_the_plain_batched_call():
    """The high voice, 64 slots, 64 x 128 ids joining in four waves of 16, one chunk of 45 frames between the waves: every
    utterance's concatenated chunks against the plain batched call of all 64 on the same injected noise, at the bound of
    the f32 path between two summation orders (a wave's join and the whole call are different batch sizes). The frame
    counts agree under the guard of tests/test_gpu_stream_batch.py: none of the 8192 durations is within 1e-4 of an integer
    before the ceil, five times the distance at which another summation order can flip one."""
    from oracle import vits_oracle as O
    from piper_amd.engine import Engine
    cfg = W.preset("high")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), device=0)
    B, T, chunk = 64, 128, 45
    ids = [W.synthetic_phoneme_ids(T, 60 + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(B)]
    rng = np.random.default_rng(64)
    nw = rng.standard_normal((B, 2, T)).astype(np.float32)
    nz = rng.standard_normal((B, cfg.inter, 512)).astype(np.float32)
    wt = O.to_torch(w)
    dist = 1.0
    for i in range(B):
        _, wv = O.durations_only(wt, cfg, ids[i], G.SCALES, nw[i], return_w=True)
        dist = min(dist, float(np.min(np.abs(wv - np.round(wv)))))
    print(f"\n[high 64 x 128] smallest distance of a pre-ceil duration from an integer: {dist:.3g}")
    assert dist >= 1e-4, dist
    full = eng.synthesize_batch(ids, G.SCALES, noise_w=nw, noise_z=nz)
    assert int(full.frames.max()) <= 512
    per = [[] for _ in range(B)]
    with eng.stream_pool(B, 512) as pool:
        calls = 0
        for wave in range(4):
            lo, hi = 16 * wave, 16 * wave + 16
            assert pool.join(ids[lo:hi], G.SCALES, noise_w=nw[lo:hi], noise_z=nz[lo:hi]) == list(range(lo, hi))
            out = pool.next(chunk)
            calls += 1
            assert sorted(out) == list(range(hi)), wave           # wave w gets its frames [0, 45) at the call after its join
            for s, c in out.items():
                per[s].append(c)
        assert np.array_equal(pool.frames, full.frames)
        while True:
            out = pool.next(chunk)
            if not out:
                break
            calls += 1
            for s, c in out.items():
                per[s].append(c)
        assert np.array_equal(pool.frames_done, full.frames) and pool.free_slots == list(range(B))
    assert calls == max(b // 16 + -(-int(full.frames[b]) // chunk) for b in range(B))      # wave w begins at call w + 1
    worst = 0.0
    for b in range(B):
        assert len(per[b]) == -(-int(full.frames[b]) // chunk), b
        cat = np.concatenate([a for a, _ in per[b]])
        assert cat.shape == full.audio[b].shape, b
        worst = max(worst, float(np.max(np.abs(cat - full.audio[b]))))
        for k, (a, p) in enumerate(per[b]):
            assert np.array_equal(O.audio_float_to_int16(a), p), (b, k)
    print(f"\n[high 64 slots, 4 waves of 16 x 128 ids] frames {int(full.frames.min())}..{int(full.frames.max())}, {calls} calls: "
          f"max |chunks - whole call| {worst:.3g}")
    assert worst < G.TIGHT_AUDIO_TOL, worst
    eng.close()
