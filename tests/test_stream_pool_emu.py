"""The stream pool (pe_stream_pool_*, Engine.stream_pool) on the test-only emulator build of the engine (tests/emu):
listeners join a live batch stream at arbitrary calls, finish, have their slot reused and leave, while every call is still
one batched window stage over all slots. The scenario and its references are tests/stream_pool_case.py; the inputs are the
three texts of tests/emu/stream_batch_case.py (6, 14 and 23 ids, chunks of 4 frames, injected noise) and a fourth of 14
ids, with the bounds tests/test_stream_batch_emu.py holds the lock-step stream to on the same inputs. The GPU counterpart
is tests/test_gpu_stream_pool.py (-m gpu)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine, EngineError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402

ONE_TOL, ORACLE_TOL, RMS_TOL = 1e-5, 1e-4, 1e-3          # tests/test_stream_batch_emu.py, same inputs


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _engine(emu_lib, preset):
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, 1234)
    return cfg, w, Engine(blob=W.pack_blob(cfg, w), lib=emu_lib)


def _check(eng, cfg, w, texts, halo):
    worst = P.check(eng, cfg, w, texts, P.CHUNK, P.FIRST, halo, ONE_TOL, ORACLE_TOL, RMS_TOL)
    print("\nframes %s chunks %s: worst %s" % ([x.frames for x in texts], [len(x.chunks) for x in texts], worst))
    return worst


def test_join_finish_reuse_leave(emu_lib, monkeypatch):
    """Three slots on poisoned workspaces: the 23-id text alone for two chunks, the 6- and 14-id texts join together, the
    fourth text takes the 6-id text's slot when that has finished, the 23-id listener hangs up in mid-stream; every newcomer's
    first chunk is 2 frames next to the residents' 4. Every delivered chunk is the one-utterance stream's and the oracle's."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, w, eng = _engine(emu_lib, "tiny")
    texts = P.emu_texts(cfg, False)
    pool = P.play(eng, texts, P.CHUNK, P.FIRST)
    assert pool.halo >= 8
    # the slot that was reused held a longer or shorter utterance before: really another tenant, and really ragged
    assert texts[3].slot == texts[0].slot and texts[3].frames != texts[0].frames
    assert len({x.frames for x in texts}) == 4
    _check(eng, cfg, w, texts, pool.halo)
    pool.close()
    eng.close()


def test_reused_slot_gets_its_own_speaker_and_tail(emu_lib, monkeypatch):
    """The same on the multi-speaker voice, every listener with another speaker: the reused slot's conditioning row must be
    the newcomer's, not its previous tenant's -- stale conditioning fails the bounds. Second half: a short utterance takes the
    row a long one held. No window reaches past an utterance's own frames (they are cut at its frame count), so a stale tail
    cannot show in the audio; the row is read back instead (debug tensor pool_z): the newcomer's latent, then zeros to the
    end of the row, where the old tenant's frames were before the join."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, w, eng = _engine(emu_lib, "tiny-ms")
    texts = P.emu_texts(cfg, True)
    assert len({x.sid for x in texts}) == 4
    pool = P.play(eng, texts, P.CHUNK, P.FIRST)
    assert texts[3].slot == texts[0].slot and texts[3].sid != texts[0].sid
    _check(eng, cfg, w, texts, pool.halo)
    # ... and the other way round: a SHORT utterance into the slot a long one held
    again = P.emu_texts(cfg, True)[0]
    old = eng.debug_tensor("pool_z", 0)                                         # slot 0 held the 23-id text
    assert P.join(pool, [again]) == [0] and again.frames + 8 < texts[2].frames
    F, row, z = again.frames, eng.debug_tensor("pool_z", 0), eng.debug_tensor("z", 0)
    assert old.shape == row.shape == (cfg.inter, 64) and z.shape == (cfg.inter, F)
    assert np.all(np.abs(old[:, F:texts[2].frames]).max(axis=0) > 0)            # the old tenant's frames were there
    assert np.array_equal(row[:, :F], z) and not np.any(row[:, F:]), np.abs(row[:, F:]).max()
    while True:
        before = pool.frames_done
        out = pool.next(P.CHUNK)
        if not out:
            break
        assert list(out) == [0]
        again.chunks.append(out[0])
        again.sizes.append(int(pool.frames_done[0] - before[0]))
    from oracle import vits_oracle as O
    wt = O.to_torch(w)
    o = O.synthesize(wt, cfg, again.ids, again.scales, again.nw, again.nz, sid=again.sid, keep=True)
    ref = O.stream_chunks(wt, cfg, o["z"], P.CHUNK, pool.halo, sid=again.sid)
    one = list(eng.stream(again.ids, again.scales, sid=again.sid, chunk_frames=P.CHUNK, noise_w=again.nw, noise_z=again.nz))
    assert len(ref) == len(one) == len(again.chunks) == -(-again.frames // P.CHUNK)
    for k, ((a, p), (a1, _), (ra, rp)) in enumerate(zip(again.chunks, one, ref)):
        assert np.array_equal(O.audio_float_to_int16(a), p), k
        assert np.max(np.abs(a - a1)) < ONE_TOL and np.max(np.abs(a - ra)) < ORACLE_TOL, k
        assert P.pcm_rms(p, rp) <= RMS_TOL, k
    pool.close()
    eng.close()


def _big_batch(cfg):
    """Four utterances, one of 136 ids at a slow rate: more utterances, more ids and more frames than anything the engine has
    seen when it runs -- both workspaces grow (and are poisoned again)."""
    ids = [W.synthetic_phoneme_ids(T, 90 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate((136, 3, 4, 5))]
    rng = np.random.default_rng(91)
    nw = rng.standard_normal((4, 2, 136)).astype(np.float32)
    nz = rng.standard_normal((4, cfg.inter, 700)).astype(np.float32)
    return ids, (0.667, 1.25, 0.8), nw, nz


def test_pool_survives_every_other_call(emu_lib, monkeypatch):
    """Between two chunks: a batched call that grows both workspaces, a lock-step batch stream drained to its end, a
    one-utterance stream, a warm-up. The pool's later chunks still meet the bounds of the first test, and the intervening
    calls give what they give on a fresh engine."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, w, eng = _engine(emu_lib, "tiny")
    _, _, fresh = _engine(emu_lib, "tiny")
    texts = P.emu_texts(cfg, False)
    bids, bsc, bnw, bnz = _big_batch(cfg)
    kids, knw, knz = K.inputs(cfg)
    seen = {}

    def hook(k, pool):
        if k == 4:
            seen["big"] = eng.synthesize_batch(bids, bsc, noise_w=bnw, noise_z=bnz)
        elif k == 6:
            seen["lock"] = K.drain(eng, kids, knw, knz)[0]
        elif k == 7:
            seen["one"] = list(eng.stream(kids[1], (0.3, 0.8, 0.5), chunk_frames=5, noise_w=knw[1], noise_z=knz[1]))
            eng.warmup(max_batch=5, max_ids=140, frames_per_id=2.0)

    pool = P.play(eng, texts, P.CHUNK, P.FIRST, hook=hook)
    assert set(seen) == {"big", "lock", "one"}
    big = seen["big"]
    assert len(bids) > pool.slots and max(len(x) for x in bids) > 128 and int(big.frames.max()) > 256, big.frames
    _check(eng, cfg, w, texts, pool.halo)
    want = fresh.synthesize_batch(bids, bsc, noise_w=bnw, noise_z=bnz)
    assert np.array_equal(want.frames, big.frames)
    for b in range(len(bids)):
        assert np.array_equal(want.audio[b], big.audio[b]) and np.array_equal(want.pcm[b], big.pcm[b]), b
    lock = K.drain(fresh, kids, knw, knz)[0]
    assert [len(c) for c in lock] == [len(c) for c in seen["lock"]]
    for cb, wb in zip(seen["lock"], lock):
        for (a, p), (wa, wp) in zip(cb, wb):
            assert np.array_equal(a, wa) and np.array_equal(p, wp)
    one = list(fresh.stream(kids[1], (0.3, 0.8, 0.5), chunk_frames=5, noise_w=knw[1], noise_z=knz[1]))
    assert len(one) == len(seen["one"]) and all(np.array_equal(a, b) and np.array_equal(p, q)
                                                for (a, p), (b, q) in zip(one, seen["one"]))
    pool.close()
    eng.close()
    fresh.close()


def _c_args(ids, scales, sids=None):
    flat = np.ascontiguousarray(np.concatenate(ids), np.int64)
    off = np.concatenate([[0], np.cumsum([len(x) for x in ids])]).astype(np.int64)
    sc = np.ascontiguousarray(scales, np.float32)
    sd = None if sids is None else np.ascontiguousarray(sids, np.int64)
    p64, pf = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    return dict(keep=(flat, off, sc, sd), ids=flat.ctypes.data_as(p64), off=off.ctypes.data_as(p64),
                sc=sc.ctypes.data_as(pf), sids=None if sd is None else sd.ctypes.data_as(p64))


def test_errors_leave_the_pool_unchanged(emu_lib, monkeypatch):
    """Every refused call gives a non-zero code and its message and leaves the pool exactly as it was: the scenario with one
    refused call after every chunk delivers what it delivers undisturbed (the first test holds that to its references)."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, w, eng = _engine(emu_lib, "tiny-ms")
    lib, h = emu_lib, eng._h
    clean = P.emu_texts(cfg, True)
    P.play(eng, clean, P.CHUNK, P.FIRST).close()
    ch = L.PeStreamChunk()
    slot_of, frames = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    halo = C.c_int32()
    t = P.emu_texts(cfg, True)
    a1 = _c_args([t[3].ids], [t[3].scales], [t[3].sid])
    a2 = _c_args([t[0].ids, t[1].ids], [t[0].scales, t[1].scales], [t[0].sid, t[1].sid])
    nan = _c_args([t[3].ids], [(0.3, float("inf"), 0.5)], [t[3].sid])
    slow = _c_args([t[2].ids], [(0.5, 0.66, 1.0)], [t[2].sid])            # three times text 2's frames: over max_frames

    def fails(rc, text):
        assert rc != 0 and text in lib.pe_last_error().decode(), lib.pe_last_error()

    def no_pool():
        fails(lib.pe_stream_pool_next(h, P.CHUNK, None, 1, C.byref(ch)), "no stream pool")
        fails(lib.pe_stream_pool_join(h, a1["ids"], a1["off"], 1, a1["sc"], a1["sids"], None, slot_of, frames), "no stream pool")
        fails(lib.pe_stream_pool_leave(h, 0), "no stream pool")
        fails(lib.pe_stream_pool_close(h), "no stream pool")

    no_pool()                                                             # after close
    _, _, never = _engine(emu_lib, "tiny-ms")
    fails(lib.pe_stream_pool_next(never._h, P.CHUNK, None, 1, C.byref(ch)), "no stream pool")      # before any open
    fails(lib.pe_stream_pool_join(never._h, a1["ids"], a1["off"], 1, a1["sc"], a1["sids"], None, slot_of, frames), "no stream pool")
    fails(lib.pe_stream_pool_leave(never._h, 0), "no stream pool")
    never.close()
    fails(lib.pe_stream_pool_open(h, 0, 48, C.byref(halo)), "slots must be in")
    fails(lib.pe_stream_pool_open(h, 3, 0, C.byref(halo)), "max_frames must be in")
    no_pool()
    tried = set()

    def hook(k, pool):
        state = (pool.frames.tolist(), pool.frames_done.tolist(), pool.free_slots)
        free = len(state[2])
        fails(lib.pe_stream_pool_open(h, 3, 48, C.byref(halo)), "already open")
        fails(lib.pe_stream_pool_next(h, 0, None, 1, C.byref(ch)), "chunk_frames must be >= 1")
        fails(lib.pe_stream_pool_join(h, a1["ids"], a1["off"], 0, a1["sc"], a1["sids"], None, slot_of, frames), "batch size must be in")
        fails(lib.pe_stream_pool_join(h, a1["ids"], a1["off"], 1, nan["sc"], a1["sids"], None, slot_of, frames),
              "utterance 0: length_scale is not finite")
        fails(lib.pe_stream_pool_join(h, None, a1["off"], 1, a1["sc"], a1["sids"], None, slot_of, frames), "null argument")
        fails(lib.pe_stream_pool_leave(h, 3), "outside")
        if free == 0:
            fails(lib.pe_stream_pool_join(h, a1["ids"], a1["off"], 1, a1["sc"], a1["sids"], None, slot_of, frames),
                  "0 free slots, 1 utterances")
            tried.add("full")
        if free == 1:
            fails(lib.pe_stream_pool_join(h, a2["ids"], a2["off"], 2, a2["sc"], a2["sids"], None, slot_of, frames),
                  "1 free slots, 2 utterances")
            fails(lib.pe_stream_pool_leave(h, state[2][0]), "is free")
            # refused after the text encoder, the durations and the flow have run over the workspaces
            fails(lib.pe_stream_pool_join(h, slow["ids"], slow["off"], 1, slow["sc"], slow["sids"], None, slot_of, frames),
                  "the stream pool holds at most 48")
            tried.add("one free")
        if free == 2 and k > 2:
            bad = np.array(t[3].ids, np.int64)
            bad[3] = cfg.n_vocab
            with pytest.raises(EngineError, match="outside"):
                pool.join([bad], t[3].scales, sids=[t[3].sid])
            with pytest.raises(EngineError, match="speaker id outside"):
                pool.join([t[3].ids], t[3].scales, sids=[cfg.n_speakers])
            tried.add("upload")
        assert (pool.frames.tolist(), pool.frames_done.tolist(), pool.free_slots) == state

    texts = P.emu_texts(cfg, True)
    pool = P.play(eng, texts, P.CHUNK, P.FIRST, hook=hook)
    assert tried == {"full", "one free", "upload"}, tried
    for x, c in zip(texts, clean):
        assert x.sizes == c.sizes and x.frames == c.frames, x.name
        for (a, p), (ca, cp) in zip(x.chunks, c.chunks):
            assert np.array_equal(a, ca) and np.array_equal(p, cp), x.name
    pool.close()
    no_pool()
    # a pool opened again on the handle is whole
    x = P.emu_texts(cfg, True)[1]
    with eng.stream_pool(2, 48) as pool2:
        assert P.join(pool2, [x]) == [0]
        got = _drain(pool2)[0]
    one = list(eng.stream(x.ids, x.scales, sid=x.sid, chunk_frames=P.CHUNK, noise_w=x.nw, noise_z=x.nz))
    assert len(got) == len(one) == -(-x.frames // P.CHUNK)
    assert all(np.max(np.abs(a - b)) < ONE_TOL for (a, _), (b, _) in zip(got, one))
    no_pool()
    eng.close()


def _drain(pool, **kw):
    per = {}
    while True:
        out = pool.next(P.CHUNK, **kw)
        if not out:
            return per
        for s, c in out.items():
            per.setdefault(s, []).append(c)


def test_pcm_alone_and_destroy_with_an_open_pool(emu_lib, monkeypatch):
    """want_audio = False delivers the same int16 and no floats; destroying the handle frees an open pool."""
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, w, eng = _engine(emu_lib, "tiny")
    t = P.emu_texts(cfg, False)
    with eng.stream_pool(2, 48) as pool:
        assert P.join(pool, t[:2]) == [0, 1]
        a = _drain(pool)
    pool = eng.stream_pool(2, 48)                                          # left open
    assert P.join(pool, t[:2]) == [0, 1]
    b = _drain(pool, want_audio=False)
    assert sorted(a) == sorted(b) == [0, 1]
    for s in a:
        assert len(a[s]) == len(b[s]) == -(-t[s].frames // P.CHUNK)
        for (fa, p), (fb, q) in zip(a[s], b[s]):
            assert fa is not None and fb is None and np.array_equal(p, q)
    assert P.join(pool, t[2:3]) == [0] and len(pool.next(P.CHUNK)) == 1      # in mid-stream when the handle goes
    eng.close()


def test_pool_does_not_depend_on_wave_order():
    """The multi-speaker scenario once per fiber order of the emulator (ascending, EMU_ORDER=reverse, =shuffle), each in a
    process of its own: identical int16 output, so stream_adopt_kernel and the window stage on pool rows do not depend on the
    order in which waves run."""
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    outs = []
    for order in ("", "reverse", "shuffle"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_pool_case.py")], capture_output=True,
                           text=True, timeout=900, env=dict(os.environ, EMU_ORDER=order, PIPER_HIP_DEBUG_POISON="1"))
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert outs[0]["pcm_sha256"] == outs[1]["pcm_sha256"] == outs[2]["pcm_sha256"], outs
    assert outs[0]["sizes"] == outs[1]["sizes"] == outs[2]["sizes"] and min(len(s) for s in outs[0]["sizes"]) >= 2
