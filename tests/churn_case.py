"""Settings churn does not leak into results: the case shared by tests/test_churn_emu.py and tests/test_gpu_churn.py.

Every delivery feature keeps side buffers of its own next to the workspaces -- the resampler's table and rows, the loudness
blocks, the true-peak table, the limiter's window and rows, the pool's latents, the gain blocks. Their lifetime is what this
pins: an engine whose settings were changed again and again between its calls, so that every one of those buffers was
allocated, regrown or replaced, must deliver bit for bit what a fresh engine delivers that was given the final settings once.

Tiny voice, synthetic weights, injected noise. Three whole-utterance calls: B = 1 with 8 ids, B = 3 with 13 / 5 / 9 ids (the
workspaces and every row block regrow), B = 2 with 13 / 8 ids.

    E1  call 1 at the defaults
        output rate 16000 (the tiny voice's own rate: still off), then 48000, so that a resampling table exists for the next
        step to replace; loudness on at -23 LUFS / -1 dB under the sample-peak ceiling
        call 2
        output rate 22050; true-peak ceiling; limiter on at 5 ms; stream gain running; a pool of 2 slots opened (its
        sizing uploads the 5 ms window); limiter window 3 ms; one join (its sizing replaces the window's table, which drops
        the graphs), one chunk, the pool closed; stream gain back to the default
        call 3, and call 3 again
    E2  output rate 22050, loudness -23 / -1, true peak, limiter 3 ms, once; then calls 1, 2, 3

Call 3's floats, int16, frame and sample counts and the three reports are equal bit for bit, and E1's second call 3 captures
no graph. (The new window is taken up by the join, not by call 3: a table replaced while a call sizes its buffers drops the
graphs that call has just captured, and its repeat would capture them again.)"""
import numpy as np

from piper_amd import weights as W

SCALES = (0.667, 0.5, 0.8)
CALLS = ((8,), (13, 5, 9), (13, 8))
TARGET, CEILING = -23.0, -1.0
FINAL_RATE, FINAL_MS = 22050, 3.0


def inputs(cfg, lens, seed):
    ids = [W.synthetic_phoneme_ids(T, seed + i, id_max=cfg.n_vocab - 1) for i, T in enumerate(lens)]
    rng = np.random.default_rng(seed)
    Tm = max(lens)
    return (ids, rng.standard_normal((len(lens), 2, Tm)).astype(np.float32),
            rng.standard_normal((len(lens), cfg.inter, 48 * Tm + 64)).astype(np.float32))


def call(eng, cfg, k):
    ids, nw, nz = inputs(cfg, CALLS[k], 300 + 10 * k)
    return eng.synthesize_batch(ids, SCALES, noise_w=nw, noise_z=nz)


def reports(eng):
    return [np.array(v) for v in eng.last_loudness() + (eng.last_true_peak(),) + eng.last_limiter()]


def churned(eng, cfg):
    """E1: returns (call 3, its reports, captures after call 3, the repeat, its reports, captures after the repeat)."""
    r1 = call(eng, cfg, 0)
    assert eng.output_rate == cfg.sample_rate
    eng.set_output_rate(16000)
    eng.set_output_rate(48000)
    eng.set_loudness(TARGET, CEILING)
    r2 = call(eng, cfg, 1)
    assert eng.last_loudness()[0].size == 3 and eng.last_limiter()[0].size == 0
    assert all(a.size == -(-int(f) * cfg.hop * 48000 // cfg.sample_rate) for a, f in zip(r2.audio, r2.frames))
    eng.set_output_rate(FINAL_RATE)
    eng.set_loudness(TARGET, CEILING, true_peak=True)
    eng.set_loudness(TARGET, CEILING, true_peak=True, limiter=True, limiter_ms=5.0)
    eng.set_stream_gain("running", peak=0.05, ramp_ms=2.0)
    ids, nw, nz = inputs(cfg, CALLS[0], 300)
    with eng.stream_pool(2, int(r1.frames[0])) as pool:
        eng.set_loudness(TARGET, CEILING, true_peak=True, limiter=True, limiter_ms=FINAL_MS)
        assert pool.join(ids, SCALES, noise_w=nw, noise_z=nz) == [0]
        got = pool.next(chunk_frames=4)
        assert list(got) == [0] and got[0][1].size > 0
        assert eng.stream_last_gains()[0].size == 2
    eng.set_stream_gain("chunk")
    r3 = call(eng, cfg, 2)
    rep3, c3 = reports(eng), eng.graph_stats[1]
    again = call(eng, cfg, 2)
    return r3, rep3, c3, again, reports(eng), eng.graph_stats[1]


def fresh(eng, cfg):
    """E2: returns (call 3, its reports)."""
    eng.set_output_rate(FINAL_RATE)
    eng.set_loudness(TARGET, CEILING, true_peak=True, limiter=True, limiter_ms=FINAL_MS)
    call(eng, cfg, 0)
    call(eng, cfg, 1)
    r3 = call(eng, cfg, 2)
    return r3, reports(eng)


def same(a, ra, b, rb, what):
    assert np.array_equal(a.frames, b.frames), (what, a.frames, b.frames)
    assert len(a.audio) == len(b.audio) == len(CALLS[2])
    for k, (x, y) in enumerate(zip(a.audio + a.pcm, b.audio + b.pcm)):
        assert x.size and x.dtype == y.dtype and x.shape == y.shape, (what, k, x.shape, y.shape)      # (equal sample offsets)
        assert np.array_equal(x.view(np.int32 if x.dtype == np.float32 else np.int16), y.view(np.int32 if y.dtype == np.float32 else np.int16)), (what, k)
    assert len(ra) == len(rb) == 8
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert x.size == len(CALLS[2]) and x.dtype == y.dtype, (what, "report", k, x.size)
        assert np.array_equal(x.view(np.int32), y.view(np.int32)), (what, "report", k, x, y)


def check(make_engine):
    """make_engine() -> (cfg, weights, engine), with the environment already as the variant wants it."""
    cfg, _, e1 = make_engine()
    _, _, e2 = make_engine()
    r3, rep3, c3, again, rep_again, c_again = churned(e1, cfg)
    f3, frep = fresh(e2, cfg)
    for e in (e1, e2):
        assert e.output_rate == FINAL_RATE and e.loudness() == (TARGET, CEILING) and e.loudness_ceiling()[0] == 1
        assert e.loudness_limiter()[:2] == (True, FINAL_MS) and e.stream_gain[0] == "chunk"
    assert all(a.size == -(-int(f) * cfg.hop * FINAL_RATE // cfg.sample_rate) for a, f in zip(r3.audio, r3.frames))
    same(r3, rep3, f3, frep, "churned against fresh")
    same(again, rep_again, r3, rep3, "the repeat")
    assert c_again == c3, (c3, c_again)
    e1.close()
    e2.close()
