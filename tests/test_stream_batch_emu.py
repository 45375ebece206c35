"""Batch streaming (pe_stream_begin_batch / pe_stream_next_batch, Engine.stream_batch) on the test-only emulator build of
the engine (tests/emu): B utterances begun together, every call returns the next chunk of each, decoded as one batched
generator pass on exact-halo windows and peak-normalised per chunk on the device. Chunk k of utterance b is what the
one-utterance stream gives for that utterance alone; utterances finish at different calls. The GPU counterpart is
tests/test_gpu_stream_batch.py (-m gpu)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import vits_oracle as O
from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import stream_batch_case as K                            # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _check_ragged_stream(eng, cfg, w, ids, nw, nz, sids, scales=K.SCALES):
    """Everything the ragged case pins, per utterance: chunk counts, the unchunked waveform of the same batched call, the
    one-utterance stream, the int16 rule on the chunk's own floats, the oracle's chunked decode of the oracle's latent."""
    B = len(ids)
    per, done = K.drain(eng, ids, nw, nz, sids=sids, scales=scales)
    frames, halo = eng.stream_frames.copy(), eng.stream_halo
    assert halo >= 8 and frames.shape == (B,)
    nchunks = [-(-int(f) // K.CHUNK) for f in frames]
    assert [len(c) for c in per] == nchunks
    assert min(nchunks) + 3 <= max(nchunks), nchunks          # really ragged: the shortest is done 3 chunks early
    assert len(done) == max(nchunks)
    for prev, cur in zip([np.zeros(B, np.int32)] + done[:-1], done):
        assert np.all(cur >= prev) and np.all(cur <= frames)
        assert np.array_equal(cur, np.minimum(frames, prev + K.CHUNK))
    assert np.array_equal(done[-1], frames) and np.array_equal(eng.stream_frames_done, frames)
    full = eng.synthesize_batch(ids, scales, sids=sids, noise_w=nw, noise_z=nz)
    assert np.array_equal(full.frames, frames)
    wt = O.to_torch(w)
    for b in range(B):
        sid = None if sids is None else sids[b]
        sc = tuple(float(v) for v in scales[b])
        cat = np.concatenate([a for a, _ in per[b]])
        assert cat.shape == full.audio[b].shape, b
        assert np.max(np.abs(cat - full.audio[b])) < 1e-5, b
        one = list(eng.stream(ids[b], sc, sid=sid, chunk_frames=K.CHUNK, noise_w=nw[b], noise_z=nz[b]))
        assert eng.stream_frames == frames[b] and len(one) == len(per[b]), b
        o = O.synthesize(wt, cfg, ids[b], sc, nw[b], nz[b], sid=sid, keep=True)
        ref = O.stream_chunks(wt, cfg, o["z"], K.CHUNK, halo, sid=sid)
        assert len(ref) == len(per[b]), b
        for k, ((a, p), (a1, p1), (ra, rp)) in enumerate(zip(per[b], one, ref)):
            assert a.shape == a1.shape == ra.shape, (b, k)
            assert np.max(np.abs(a - a1)) < 1e-5, (b, k)
            assert p.dtype == np.int16 and np.array_equal(O.audio_float_to_int16(a), p), (b, k)
            assert np.max(np.abs(a - ra)) < 1e-4, (b, k)
            assert np.sqrt(np.mean(((p.astype(np.float64) - rp) / 32767.0) ** 2)) <= 1e-3, (b, k)
    return per


def test_ragged_batch_stream_equals_every_utterance_alone(emu_lib, monkeypatch):
    """Three utterances of 6, 14 and 23 ids with three scale triples, chunks of 4 frames, the activation workspaces
    poisoned with NaN patterns before use: a window column read without having been written shows up in the output."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    ids, nw, nz = K.inputs(cfg)
    _check_ragged_stream(eng, cfg, w, ids, nw, nz, None)
    eng.close()


def test_ragged_batch_stream_keeps_every_utterance_its_speaker(emu_lib, monkeypatch):
    """The same on a multi-speaker voice with three different speakers: the generator's conditioning is indexed by
    utterance, so a batch compacted to the unfinished utterances would give the late chunks the wrong voice."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg = W.preset("tiny-ms")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    ids, nw, nz = K.inputs(cfg)
    _check_ragged_stream(eng, cfg, w, ids, nw, nz, list(K.SIDS), K.SCALES_MS)
    eng.close()


def test_chunk_size_may_change_from_call_to_call(emu_lib):
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    ids, nw, nz = K.inputs(cfg)
    full = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    sizes = (3, 5, 64)
    per, done = K.drain(eng, ids, nw, nz, chunk_frames=lambda k: sizes[min(k, 2)])
    want = np.zeros(len(ids), np.int32)
    for k, d in enumerate(done):
        want = np.minimum(eng.stream_frames, want + sizes[min(k, 2)])
        assert np.array_equal(d, want), k
    assert len(done) == 3 and np.array_equal(done[-1], full.frames)
    for b in range(len(ids)):
        cat = np.concatenate([a for a, _ in per[b]])
        assert cat.shape == full.audio[b].shape and np.max(np.abs(cat - full.audio[b])) < 1e-5, b
        assert all(np.array_equal(O.audio_float_to_int16(a), p) for a, p in per[b])
    # a chunk larger than every utterance: everything in one call, which is then the unchunked result, int16 included
    # (with per-launch profiling on: the window stage's own kernels have rows of their own, the whole-window pcm16_kernel
    # is not part of it)
    eng.profile_enable(2)
    eng.profile_reset()
    per, done = K.drain(eng, ids, nw, nz, chunk_frames=100000)
    rows = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
    eng.profile_enable(0)
    assert rows.get("window_gather_kernel") == rows.get("chunk_peak_kernel") == rows.get("chunk_pcm_kernel") == 1, rows
    assert "pcm16_kernel" not in rows and "window_copy_kernel" not in rows, rows
    assert len(done) == 1 and np.array_equal(done[0], full.frames)
    for b in range(len(ids)):
        assert len(per[b]) == 1 and per[b][0][0].shape == full.audio[b].shape
        assert np.max(np.abs(per[b][0][0] - full.audio[b])) < 1e-5
        assert np.array_equal(O.audio_float_to_int16(per[b][0][0]), per[b][0][1])
    eng.close()


def test_pcm_alone_is_the_pcm_of_the_run_with_floats(emu_lib):
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    ids, nw, nz = K.inputs(cfg)
    with_audio, _ = K.drain(eng, ids, nw, nz, want_audio=True)
    pcm_only, _ = K.drain(eng, ids, nw, nz, want_audio=False)
    for b in range(len(ids)):
        assert len(with_audio[b]) == len(pcm_only[b]) > 0
        for (a, p), (a0, p0) in zip(with_audio[b], pcm_only[b]):
            assert a is not None and a0 is None            # pe_stream_chunk.audio is NULL
            assert np.array_equal(p, p0)
    eng.close()


def _c_args(ids, scales, sids=None):
    flat = np.ascontiguousarray(np.concatenate(ids), np.int64)
    off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int64)
    sc = np.ascontiguousarray(scales, np.float32)
    sd = None if sids is None else np.ascontiguousarray(sids, np.int64)
    p64, pf = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    return dict(keep=(flat, off, sc, sd), ids=flat.ctypes.data_as(p64), off=off.ctypes.data_as(p64),
                sc=sc.ctypes.data_as(pf), sids=None if sd is None else sd.ctypes.data_as(p64))


def test_errors_leave_the_handle_and_a_running_stream_usable(emu_lib):
    """Every argument error gives a non-zero code and its message, and the handle still completes the ragged stream of the
    first test (here on the multi-speaker voice, with its speakers, so that a speaker id can be out of range): errors that
    are refused before the engine is touched leave even a stream in progress intact; a refused upload ends it, and the
    next stream is complete again. Another synthesis call ends a batch stream."""
    cfg = W.preset("tiny-ms")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)
    ids, nw, nz = K.inputs(cfg)
    sids = list(K.SIDS)
    lib, h = emu_lib, eng._h
    ch = L.PeStreamChunk()
    frames = (C.c_int32 * 3)()
    halo = C.c_int32()

    def fails(rc, text):
        assert rc != 0 and text in lib.pe_last_error().decode(), lib.pe_last_error()

    fails(lib.pe_stream_next_batch(h, K.CHUNK, 1, C.byref(ch)), "no batch stream")
    one_before = list(eng.stream(ids[1], (0.3, 0.18, 0.5), sid=3, chunk_frames=K.CHUNK, noise_w=nw[1], noise_z=nz[1]))
    fails(lib.pe_stream_next_batch(h, K.CHUNK, 1, C.byref(ch)), "no batch stream")
    want, _ = K.drain(eng, ids, nw, nz, sids=sids, scales=K.SCALES_MS)

    def same(per):
        assert [len(c) for c in per] == [len(c) for c in want]
        for cb, wb in zip(per, want):
            for (a, p), (wa, wp) in zip(cb, wb):
                assert np.array_equal(a, wa) and np.array_equal(p, wp)

    # a stream in progress, one refused call between every two chunks
    a = _c_args(ids, K.SCALES_MS, sids)
    bad_scale = K.SCALES_MS.copy()
    bad_scale[1, 1] = np.nan
    nan = _c_args(ids, bad_scale, sids)
    refused = [
        lambda: fails(lib.pe_stream_begin_batch(h, None, a["off"], 3, a["sc"], a["sids"], None, frames, C.byref(halo)), "null argument"),
        lambda: fails(lib.pe_stream_begin_batch(h, a["ids"], None, 3, a["sc"], a["sids"], None, frames, C.byref(halo)), "null argument"),
        lambda: fails(lib.pe_stream_begin_batch(h, a["ids"], a["off"], 3, None, a["sids"], None, frames, C.byref(halo)), "null scales"),
        lambda: fails(lib.pe_stream_begin_batch(h, a["ids"], a["off"], 0, a["sc"], a["sids"], None, frames, C.byref(halo)), "batch size must be in"),
        lambda: fails(lib.pe_stream_begin_batch(h, a["ids"], a["off"], 3, nan["sc"], a["sids"], None, frames, C.byref(halo)), "utterance 1: length_scale is not finite"),
        lambda: fails(lib.pe_stream_next_batch(h, 0, 1, C.byref(ch)), "chunk_frames must be >= 1"),
        lambda: fails(lib.pe_stream_next_batch(h, K.CHUNK, 1, None), "null argument"),
    ]
    per = [[] for _ in ids]
    for k, item in enumerate(eng.stream_batch(ids, K.SCALES_MS, sids=sids, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)):
        for b, (fa, p) in enumerate(item):
            if p.size:
                per[b].append((fa, p))
        if k < len(refused):
            refused[k]()
    assert k + 1 >= len(refused)
    same(per)
    # refused inside the upload: the inputs are half replaced, the stream is over -- and the next one is whole
    bad_ids = [np.array(x, np.int64) for x in ids]
    bad_ids[2][5] = cfg.n_vocab
    with pytest.raises(EngineError, match="outside"):
        next(eng.stream_batch(bad_ids, K.SCALES_MS, sids=sids, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz))
    fails(lib.pe_stream_next_batch(h, K.CHUNK, 1, C.byref(ch)), "no batch stream")
    same(K.drain(eng, ids, nw, nz, sids=sids, scales=K.SCALES_MS)[0])
    with pytest.raises(EngineError, match="speaker id outside"):
        next(eng.stream_batch(ids, K.SCALES_MS, sids=[1, cfg.n_speakers, 0], chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz))
    # ... and a synthesis call between two chunks ends the stream: an error, not stale data
    gen = eng.stream_batch(ids, K.SCALES_MS, sids=sids, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)
    first, second = next(gen), next(gen)
    for b in range(3):
        assert np.array_equal(first[b][1], want[b][0][1])
        if len(want[b]) > 1:
            assert np.array_equal(second[b][1], want[b][1][1])
    eng.synthesize(ids[0], (0.3, 0.18, 0.5), sid=2)
    with pytest.raises(EngineError, match="no batch stream"):
        next(gen)
    same(K.drain(eng, ids, nw, nz, sids=sids, scales=K.SCALES_MS)[0])
    # the one-utterance stream of the same handle is what it was
    one_after = list(eng.stream(ids[1], (0.3, 0.18, 0.5), sid=3, chunk_frames=K.CHUNK, noise_w=nw[1], noise_z=nz[1]))
    assert len(one_after) == len(one_before)
    for (fa, p), (fb, q) in zip(one_after, one_before):
        assert np.array_equal(fa, fb) and np.array_equal(p, q)
    # the window buffer is the dead prior-noise buffer: its debug view refuses while a batch stream is live
    gen = eng.stream_batch(ids, K.SCALES_MS, sids=sids, chunk_frames=K.CHUNK, noise_w=nw, noise_z=nz)
    next(gen)
    with pytest.raises(EngineError, match="noise_z is not available"):
        eng.debug_tensor("noise_z", 0)
    gen.close()
    eng.close()


def test_batch_stream_does_not_depend_on_wave_order():
    """The ragged stream once per fiber order of the emulator (ascending, EMU_ORDER=reverse, =shuffle), each in a process of
    its own: identical int16 output, so neither the gather nor the two delivery kernels (a reduction through LDS and one
    atomic maximum per workgroup) depend on the order in which waves reach a barrier."""
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    outs = []
    for order in ("", "reverse", "shuffle"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu", "stream_batch_case.py")], capture_output=True,
                           text=True, timeout=900, env=dict(os.environ, EMU_ORDER=order))
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert outs[0]["chunks"] == [-(-f // K.CHUNK) for f in outs[0]["frames"]]
    assert outs[0]["pcm_sha256"] == outs[1]["pcm_sha256"] == outs[2]["pcm_sha256"], outs
    assert outs[0]["frames"] == outs[1]["frames"] == outs[2]["frames"]
