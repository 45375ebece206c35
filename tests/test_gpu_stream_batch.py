"""Batch streaming on the MI355X (run with -m gpu): pe_stream_begin_batch / pe_stream_next_batch through
piper_amd.engine.Engine.stream_batch against the engine's own unchunked batched call, its one-utterance stream, and the
oracle's restatement of the reference's chunked decode (oracle.stream_chunks) on the oracle's latent. The emulator
counterpart, with the ragged / zero-delivery corner cases on poisoned workspaces, is tests/test_stream_batch_emu.py."""
import numpy as np
import pytest

from piper_amd import weights as W

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3           # BASELINE.json north_star (tests/test_gpu_parity.py)
TIGHT_AUDIO_TOL = 2e-4   # the f32 path between two summation orders, max abs on the float waveform
CHUNK_TOL = 2e-5         # chunks against the engine's own unchunked waveform (tests/test_gpu_parity.py)
SCALES = (0.667, 1.0, 0.8)

CASES = {
    "medium": ((32, 48, 64, 80, 96, 104, 120, 128), 45),
    "high": ((24, 32, 48, 64), 45),
    "tiny": ((9, 17, 26, 38, 50), 7),
}

_engines = {}


def engine_for(preset, seed=1234):
    from piper_amd.engine import Engine
    if preset not in _engines:
        cfg = W.preset(preset)
        w = W.synthetic_weights(cfg, seed)
        _engines[preset] = (cfg, w, Engine(blob=W.pack_blob(cfg, w), device=0))
    return _engines[preset]


def noise_for(cfg, lens):
    """Utterance i: noise_w (2, T_i) first, then noise_z (inter, 32 T_i + 64), from default_rng(100 + i); both zero-padded
    to the batch's largest stride."""
    Tm = max(lens)
    nw = np.zeros((len(lens), 2, Tm), np.float32)
    nz = np.zeros((len(lens), cfg.inter, 32 * Tm + 64), np.float32)
    for i, T in enumerate(lens):
        rng = np.random.default_rng(100 + i)
        nw[i, :, :T] = rng.standard_normal((2, T)).astype(np.float32)
        nz[i, :, :32 * T + 64] = rng.standard_normal((cfg.inter, 32 * T + 64)).astype(np.float32)
    return nw, nz


def inputs_for(cfg, lens):
    ids = [W.synthetic_phoneme_ids(T, 60 + i, id_max=min(cfg.n_vocab - 1, 129)) for i, T in enumerate(lens)]
    return (ids,) + noise_for(cfg, lens)


def pcm_rms(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)) / 32767.0
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def drain(eng, ids, chunk, **kw):
    per = [[] for _ in ids]
    calls = 0
    for item in eng.stream_batch(ids, SCALES, chunk_frames=chunk, **kw):
        calls += 1
        for b, (a, p) in enumerate(item):
            if p.size:
                per[b].append((a, p))
    return per, calls


@pytest.mark.parametrize("preset", list(CASES))
def test_batch_stream_equals_every_utterance_alone(preset):
    """A ragged batch streamed in lock step: per utterance the chunks concatenate to the unchunked waveform of the same
    batched call (2e-5), equal the one-utterance stream chunk by chunk (2e-5), carry the int16 of their own floats bit
    for bit, and match the oracle's chunked decode of the oracle's latent (2e-4 / 1e-3 RMS). No utterance is left out."""
    from oracle import vits_oracle as O
    lens, chunk = CASES[preset]
    cfg, w, eng = engine_for(preset)
    ids, nw, nz = inputs_for(cfg, lens)
    wt = O.to_torch(w)
    # a frame count that differs from the oracle's must not be the known one-frame flip of a duration whose value before
    # the ceil sits within 2e-5 of an integer in another summation order: these inputs keep five times that distance
    dist = 1.0
    for i in range(len(lens)):
        _, wv = O.durations_only(wt, cfg, ids[i], SCALES, nw[i], return_w=True)
        dist = min(dist, float(np.min(np.abs(wv - np.round(wv)))))
    print(f"\n[{preset}] smallest distance of a pre-ceil duration from an integer: {dist:.3g}")
    assert dist >= 1e-4, dist
    per, calls = drain(eng, ids, chunk, noise_w=nw, noise_z=nz)
    frames, halo = eng.stream_frames.copy(), eng.stream_halo
    assert np.array_equal(eng.stream_frames_done, frames)
    assert calls == -(-int(frames.max()) // chunk) and len(set(-(-int(f) // chunk) for f in frames)) > 1, frames
    full = eng.synthesize_batch(ids, SCALES, noise_w=nw, noise_z=nz)
    assert np.array_equal(full.frames, frames)
    worst = dict(full=0.0, one=0.0, oracle=0.0, rms=0.0)
    for b in range(len(lens)):
        o = O.synthesize(wt, cfg, ids[b], SCALES, nw[b], nz[b], keep=True)
        assert int(frames[b]) == int(o["frames"]), (b, frames[b], o["frames"])
        assert len(per[b]) == -(-int(frames[b]) // chunk), b
        cat = np.concatenate([a for a, _ in per[b]])
        assert cat.shape == full.audio[b].shape, b
        one = list(eng.stream(ids[b], SCALES, chunk_frames=chunk, noise_w=nw[b], noise_z=nz[b]))
        ref = O.stream_chunks(wt, cfg, o["z"], chunk, halo)
        assert len(one) == len(ref) == len(per[b]), b
        worst["full"] = max(worst["full"], float(np.max(np.abs(cat - full.audio[b]))))
        for k, ((a, p), (a1, p1), (ra, rp)) in enumerate(zip(per[b], one, ref)):
            assert a.shape == a1.shape == ra.shape and p.shape == rp.shape, (b, k)
            assert np.array_equal(O.audio_float_to_int16(a), p), (b, k)
            worst["one"] = max(worst["one"], float(np.max(np.abs(a - a1))))
            worst["oracle"] = max(worst["oracle"], float(np.max(np.abs(a - ra))))
            worst["rms"] = max(worst["rms"], pcm_rms(p, rp))
    print(f"[{preset}] frames {frames.tolist()} halo {halo}: max |chunks - unchunked| {worst['full']:.3g}, "
          f"max |chunk - one-utterance chunk| {worst['one']:.3g}, max |chunk - oracle chunk| {worst['oracle']:.3g}, "
          f"worst chunk pcm rms {worst['rms']:.3g}")
    assert worst["full"] < CHUNK_TOL and worst["one"] < CHUNK_TOL, worst
    assert worst["oracle"] < TIGHT_AUDIO_TOL and worst["rms"] <= RMS_TOL, worst


def test_flagship_batch_as_a_stream_equals_the_whole_call():
    """BASELINE configs[2] as a stream: the high voice, 64 x 128 ids, noise drawn by the engine. Two fresh engines of the same
    blob and seed are both at run counter 1 (the draws depend on seed, counter, site, row and column only): one streams the
    batch in chunks of 45 frames, the other runs the whole call. The batch size is a kernel-form regime no other chunked
    test visits, so the floats are held to the bound of the f32 path between two summation orders."""
    from oracle import vits_oracle as O
    from piper_amd.engine import Engine
    cfg = W.preset("high")
    blob = W.pack_blob(cfg, W.synthetic_weights(cfg, 1234))
    ids = [W.synthetic_phoneme_ids(128, 60 + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(64)]
    e1, e2 = Engine(blob=blob, device=0), Engine(blob=blob, device=0)
    e1.set_seed(99)
    e2.set_seed(99)
    assert e1.rng_calls == e2.rng_calls == 0
    per, calls = drain(e1, ids, 45)
    full = e2.synthesize_batch(ids, SCALES)
    assert e1.rng_calls == e2.rng_calls == 1
    assert np.array_equal(e1.stream_frames, full.frames)
    assert calls == -(-int(full.frames.max()) // 45)
    worst = 0.0
    for b in range(64):
        assert len(per[b]) == -(-int(full.frames[b]) // 45), b
        cat = np.concatenate([a for a, _ in per[b]])
        assert cat.shape == full.audio[b].shape, b
        worst = max(worst, float(np.max(np.abs(cat - full.audio[b]))))
        for k, (a, p) in enumerate(per[b]):
            assert np.array_equal(O.audio_float_to_int16(a), p), (b, k)
    print(f"\n[high 64 x 128] frames {int(full.frames.min())}..{int(full.frames.max())}, {calls} chunks of 45: "
          f"max |chunks - whole call| {worst:.3g}")
    assert worst < TIGHT_AUDIO_TOL, worst
    e1.close()
    e2.close()


def test_second_batch_of_a_bucket_replays_and_existing_calls_are_untouched():
    """One captured graph per (batch, window bucket) serves every chunk of every batch: draining a second, different batch
    of the same shape buckets captures nothing. A batch stream leaves the workspaces and graphs of the existing calls
    alone: the plain batched call gives the output it gave before the streams."""
    from piper_amd.engine import Engine
    lens, chunk = CASES["medium"]
    cfg = W.preset("medium")
    eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    ids, nw, nz = inputs_for(cfg, lens)
    before = eng.synthesize_batch(ids, SCALES, noise_w=nw, noise_z=nz)
    # injected duration noise fixes the frame counts (and with them the buckets), the prior noise is the engine's: every
    # stage of the stream is a captured graph
    per1, calls1 = drain(eng, ids, chunk, noise_w=nw)
    frames1 = eng.stream_frames.copy()
    assert np.array_equal(frames1, before.frames)
    cached1, captures1 = eng.graph_stats
    # the same utterances in reverse order: another batch (every slot holds another utterance, every chunk other windows
    # and delivery ranges), the same id, frame and window buckets
    per2, calls2 = drain(eng, ids[::-1], chunk, noise_w=np.ascontiguousarray(nw[::-1]))
    cached2, captures2 = eng.graph_stats
    print(f"\n[medium x {len(lens)}] graphs cached / captured after the first stream {cached1} / {captures1}, "
          f"after the second {cached2} / {captures2}")
    assert np.array_equal(eng.stream_frames, frames1[::-1]) and calls2 == calls1
    assert [len(c) for c in per2] == [len(c) for c in per1][::-1]
    assert captures1 > 0 and captures2 == captures1 and cached2 == cached1
    after = eng.synthesize_batch(ids, SCALES, noise_w=nw, noise_z=nz)
    assert np.array_equal(after.frames, before.frames)
    for b in range(len(lens)):
        assert np.array_equal(after.audio[b], before.audio[b]) and np.array_equal(after.pcm[b], before.pcm[b]), b
    eng.close()
