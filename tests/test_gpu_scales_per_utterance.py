"""Per-utterance scales on the MI355X (run with -m gpu): one batched call whose utterances each carry their own
{noise_scale, length_scale, noise_w} triple (pe_synthesize_batch_scaled and the layers above it) computes every utterance
as a call with that triple alone would -- checked against the CPU oracle, against uniform calls of the engine itself, and
through the group and the mixed coalescer -- and, the scales being call inputs rather than graph constants, new scale
values never capture new hipGraphs. The emulator counterpart is tests/test_scales_per_utterance_emu.py."""
import json
import threading

import numpy as np
import pytest

from piper_amd import weights as W

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3
AUDIO_TOL = 2e-4

_weights = {}
_oracle = {}


def voice(preset, seed=1234):
    if preset not in _weights:
        cfg = W.preset(preset)
        _weights[preset] = (cfg, W.synthetic_weights(cfg, seed))
    return _weights[preset]


def make_engine(monkeypatch, cfg, w, env=None):
    from piper_amd import _lib as L
    from piper_amd.engine import Engine
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    return Engine(blob=W.pack_blob(cfg, w), device=0)     # the knobs are read once, at engine creation


def batch_ids(lens, seed):
    return [W.synthetic_phoneme_ids(T, 100 * seed + i, id_max=129) for i, T in enumerate(lens)]


def mixed_scales(n, seed):
    rng = np.random.default_rng(seed)
    s = np.empty((n, 3), np.float32)
    s[:, 0] = rng.uniform(0.0, 1.0, n)
    s[:, 1] = rng.uniform(0.7, 1.5, n)
    s[:, 2] = rng.uniform(0.0, 1.0, n)
    s[0, 1], s[-1, 1] = 0.7, 1.5                            # both ends of the length_scale range in every batch
    return s


def pcm_rms(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)) / 32767.0
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def lsb(a, b):
    return int(np.max(np.abs(a.astype(np.int32) - b.astype(np.int32)))) if a.size else 0


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
@pytest.mark.parametrize("lens,seed", [([96, 40, 128], 1), ([128, 3, 77, 128, 50, 19, 101, 64, 128, 33, 90, 2, 111, 60, 8, 128], 2)])
def test_mixed_scales_match_the_oracle(monkeypatch, lens, seed, mode):
    """B=3 runs as the one-graph speculative form (after a first call has set the frames-per-id estimate), B=16 as the
    two-graph form around the frame-count read-back. The duration noise is injected, the prior noise is the engine's own
    (read back per utterance for the oracle)."""
    from oracle import vits_oracle as O
    cfg, w = voice("medium")
    wt = O.to_torch(w)
    eng = make_engine(monkeypatch, cfg, w, {} if mode == "f32" else {"PIPER_HIP_MATRIX": mode})
    eng.set_seed(17)
    ids = batch_ids(lens, seed)
    sc = mixed_scales(len(lens), seed)
    rng = np.random.default_rng(seed)
    nw = rng.standard_normal((len(lens), 2, max(lens))).astype(np.float32)
    eng.synthesize_batch(ids, (0.667, 1.0, 0.8), noise_w=nw)          # sets the frames-per-id estimate
    runs0 = eng.speculation_stats[0]
    r = eng.synthesize_batch(ids, sc, noise_w=nw)
    if len(lens) <= 4:
        assert eng.speculation_stats[0] == runs0 + 1
    durs = eng.durations()
    off = np.concatenate([[0], np.cumsum(lens)])
    for i in range(len(lens)):
        s = tuple(float(v) for v in sc[i])
        nz = eng.debug_tensor("noise_z", i)
        key = (seed, i)
        o = _oracle.get(key)
        if o is None or not np.array_equal(o["nz"], nz):
            o = dict(O.synthesize(wt, cfg, ids[i], s, nw[i], nz), nz=nz)
            _oracle[key] = o
        assert np.array_equal(durs[off[i]:off[i + 1]], o["durations"]), f"utterance {i}: durations differ"
        assert r.audio[i].shape == o["audio"].shape, f"utterance {i}"
        d = float(np.max(np.abs(r.audio[i] - o["audio"])))
        assert d < AUDIO_TOL, f"utterance {i}: max |d audio| = {d}"
        assert pcm_rms(r.pcm[i], o["pcm"]) <= RMS_TOL, f"utterance {i}"
    eng.close()


def test_engine_noise_mixed_call_equals_uniform_calls(monkeypatch):
    """Engine-drawn noise at both sites: utterance k of a mixed call on a fresh engine equals utterance k of a call on a
    fresh engine with the same seed, the same ids and every utterance at triple k (same run counter, same noise rows)."""
    cfg, w = voice("medium")
    lens = [64, 128, 30, 100]
    ids = batch_ids(lens, 7)
    sc = mixed_scales(len(lens), 7)
    eng = make_engine(monkeypatch, cfg, w)
    eng.set_seed(5)
    r = eng.synthesize_batch(ids, sc)
    durs = eng.durations()
    eng.close()
    off = np.concatenate([[0], np.cumsum(lens)])
    for k in range(len(lens)):
        e = make_engine(monkeypatch, cfg, w)
        e.set_seed(5)
        u = e.synthesize_batch(ids, tuple(float(v) for v in sc[k]))
        assert np.array_equal(durs[off[k]:off[k + 1]], e.durations()[off[k]:off[k + 1]]), f"utterance {k}"
        assert r.pcm[k].shape == u.pcm[k].shape and lsb(r.pcm[k], u.pcm[k]) <= 2, f"utterance {k}"
        e.close()


def test_new_scale_values_capture_no_graphs(monkeypatch):
    """The scales are call inputs, not graph constants: once the shapes a workload takes are captured, calls with new
    per-utterance triples -- and old-API calls with new length_scale values -- replay them (0 captures). B=8 runs the
    two-graph form, whose keys are the id bucket and the frame bucket; the duration noise is fixed (injected) so that
    the frame counts are a function of length_scale, and a sweep of uniform calls over the length_scale range visits
    every frame bucket the random calls can land in."""
    cfg, w = voice("medium")
    eng = make_engine(monkeypatch, cfg, w)
    lens = [40, 33, 64, 12, 50, 64, 21, 57]
    ids = batch_ids(lens, 9)
    nw = np.random.default_rng(9).standard_normal((8, 2, 64)).astype(np.float32)
    eng.warmup(max_batch=8, max_ids=64, frames_per_id=24.0)
    for ls in np.linspace(0.7, 1.5, 81):
        eng.synthesize_batch(ids, (0.667, float(ls), 0.8), noise_w=nw)
    cached, captures = eng.graph_stats
    rng = np.random.default_rng(10)
    for _ in range(100):
        sc = np.stack([rng.uniform(0, 1, 8), rng.uniform(0.7, 1.5, 8), rng.uniform(0, 1, 8)], 1).astype(np.float32)
        eng.synthesize_batch(ids, sc, noise_w=nw)
    assert eng.graph_stats[1] == captures, (captures, eng.graph_stats)
    for _ in range(100):
        eng.synthesize_batch(ids, (float(rng.uniform(0, 1)), float(rng.uniform(0.7, 1.5)), float(rng.uniform(0, 1))),
                             noise_w=nw)
    assert eng.graph_stats[1] == captures, (captures, eng.graph_stats)
    eng.close()


def test_group_and_mixed_coalescer(monkeypatch):
    """A two-engine group on one GPU with per-utterance scales returns what one engine does, in the caller's order; the
    mixed coalescer serves eight threads with four speaking rates as ONE engine call, each request what its own B=1 call
    computes. Noise scales 0: deterministic."""
    from piper_amd.group import Coalescer, EngineGroup
    cfg, w = voice("medium")
    lens = [128, 40, 77, 9, 101, 64]
    ids = batch_ids(lens, 11)
    sc = np.zeros((len(lens), 3), np.float32)
    sc[:, 1] = [0.7, 1.5, 1.0, 1.2, 0.85, 1.35]
    eng = make_engine(monkeypatch, cfg, w)
    rs = eng.synthesize_batch(ids, sc)
    monkeypatch.setenv("PIPER_HIP_GROUP_COALESCE", "0")      # both engines take part
    grp = EngineGroup(W.pack_blob(cfg, w), [0, 0])
    rg = grp.synthesize_batch(ids, sc)
    assert sorted(set(grp.assignment(len(ids)))) == [0, 1]
    assert list(rg.frames) == list(rs.frames)
    for i in range(len(ids)):
        assert rg.pcm[i].shape == rs.pcm[i].shape and lsb(rg.pcm[i], rs.pcm[i]) <= 2, f"utterance {i}"
    grp.close()

    ids8 = batch_ids([128, 90, 128, 61, 128, 100, 77, 128], 12)
    rates = [0.7, 1.0, 1.25, 1.5]
    scales = [(0.0, rates[i % 4], 0.0) for i in range(8)]
    want = [eng.synthesize(t, s).pcm[0] for t, s in zip(ids8, scales)]
    co = Coalescer(eng, max_batch=8, max_wait_us=2000000, mix_scales=True)
    out = [None] * 8

    def work(i):
        out[i] = co.synthesize(ids8[i], scales[i])

    th = [threading.Thread(target=work, args=(i,)) for i in range(8)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert co.stats == (1, 8)
    for i, (pcm, frames, secs, bs) in enumerate(out):
        assert bs == 8 and pcm.shape == want[i].shape and lsb(pcm, want[i]) <= 2, f"request {i}"
    co.close()
    eng.close()
