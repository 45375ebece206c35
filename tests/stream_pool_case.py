"""The stream-pool scenario shared by tests/test_stream_pool_emu.py, tests/test_gpu_stream_pool.py and the wave-order child
process: listeners join a live batch stream, finish, have their slot reused, and leave (pe_stream_pool_*,
Engine.stream_pool). A scenario is four texts:

  call 1, 2   text 2 (the longest) streams alone in slot 0
  join        texts 0 and 1 (and any further ones) take slots 1, 2, ...; their first chunk is FIRST frames, every other
              chunk CHUNK frames
  ...         when text 0 (the shortest) has finished, text 3 joins -- into the lowest free slot, one that had a tenant --
              with a first chunk of FIRST
  leave       one call after text 3's first chunk, the resident with the most frames to come hangs up in mid-stream
  drain       until no slot has frames left

and the references every delivered chunk is held to: the one-utterance stream of the same engine and the oracle's chunked
decode of the oracle's latent, both on the chunk sizes the listener really got. Run as a script it plays the scenario once on
the emulator build under the fiber order EMU_ORDER names and prints one JSON line with a digest of the int16 output; with
`--gpu PRESET` it plays and checks the GPU scenario of that voice on device 0 (a child process of the split-mode test)."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from piper_amd import _lib as L, weights as W            # noqa: E402
from piper_amd.engine import Engine                      # noqa: E402


class Listener:
    def __init__(self, name, ids, scales, sid, nw, nz):
        self.name, self.ids, self.scales, self.sid = name, np.asarray(ids, np.int64), tuple(float(v) for v in scales), sid
        self.nw = np.ascontiguousarray(nw, np.float32)
        self.nz = None if nz is None else np.ascontiguousarray(nz, np.float32)      # None: the engine draws the prior noise
        self.slot, self.frames, self.left = None, None, False
        self.chunks, self.sizes = [], []                 # (float, int16) per delivered chunk, its frames


def join(pool, listeners):
    slots = pool.join([x.ids for x in listeners], np.array([x.scales for x in listeners], np.float32),
                      sids=None if listeners[0].sid is None else [x.sid for x in listeners],
                      noise_w=pad_stack([x.nw for x in listeners]), noise_z=None if listeners[0].nz is None else pad_stack([x.nz for x in listeners]))
    frames = pool.frames
    for x, s in zip(listeners, slots):
        x.slot, x.frames = s, int(frames[s])
    return slots


def pad_stack(arrs):
    n = max(a.shape[-1] for a in arrs)
    out = np.zeros((len(arrs),) + arrs[0].shape[:-1] + (n,), np.float32)
    for i, a in enumerate(arrs):
        out[i, ..., :a.shape[-1]] = a
    return out


def play(eng, texts, chunk, first, slots=None, max_frames=48, hook=None, want_audio=True, pool=None, second_order=None):
    """Plays the scenario on listeners texts[0..3] (texts[4:] join together with texts 0 and 1, in `second_order` when given);
    hook(k, pool), when given, runs after call k (1-based). Returns the pool, still open (the caller closes it), after the
    call that delivered nothing."""
    hop = eng.hop
    t0, t2, t3 = texts[0], texts[2], texts[3]
    second = [texts[0], texts[1]] + list(texts[4:])
    if second_order is not None:
        second = [second[i] for i in second_order]
    slots = slots or 1 + len(second)
    if pool is None:
        pool = eng.stream_pool(slots, max_frames)
    assert pool.free_slots == list(range(slots))
    assert join(pool, [t2]) == [0]
    on = {0: t2}
    pending = {}                                         # slot -> first chunk size
    calls = since_t3 = 0
    someone_left = False
    while True:
        calls += 1
        assert calls < 200
        before = pool.frames_done
        out = pool.next(chunk, per_slot=pending or None, want_audio=want_audio)
        done = pool.frames_done
        if not out:
            assert np.array_equal(done, before)
            break
        for s in range(slots):
            x = on.get(s)
            got = int(done[s] - before[s])
            if x is None or x.left or got == 0:
                assert s not in out and got == 0, (calls, s)
                continue
            a, p = out[s]
            assert p.size == got * hop and (a is None or a.shape == p.shape), (calls, s)
            assert got == min(pending.get(s, chunk), x.frames - int(before[s])), (calls, s)
            x.chunks.append((a, p))
            x.sizes.append(got)
        pending = {}
        if hook is not None:
            hook(calls, pool)
        if calls == 2:
            assert join(pool, second) == list(range(1, 1 + len(second)))
            for x in second:
                on[x.slot] = x
                pending[x.slot] = first
        if t3.slot is not None:
            since_t3 += 1
            if since_t3 == 2:
                # one listener hangs up in mid-stream: the resident with the most frames still to come (the newcomer
                # itself only if nobody else is left)
                live = [x for x in on.values() if not x.left and done[x.slot] < x.frames]
                assert live
                x = max(live, key=lambda x: (x is not t3, x.frames - int(done[x.slot])))
                assert x.slot not in pool.free_slots
                pool.leave(x.slot)
                x.left = someone_left = True
                assert x.slot in pool.free_slots and pool.frames_done[x.slot] == done[x.slot]
        elif t0.slot is not None and done[t0.slot] == t0.frames:
            # a finished slot is free, its frames_done readable; the newcomer takes the lowest free slot, a reused one
            free = pool.free_slots
            assert t0.slot in free and pool.frames[t0.slot] == t0.frames and all(s in on for s in free)
            assert join(pool, [t3]) == [free[0]]
            on[t3.slot] = t3
            pending = {t3.slot: first}
            assert pool.frames_done[t3.slot] == 0 and t3.slot not in pool.free_slots
    assert t3.slot is not None and someone_left
    assert pool.free_slots == list(range(slots))
    return pool


def expected_sizes(frames, first, chunk):
    sizes, f = [], 0
    while f < frames:
        c = min(first if (not sizes and first) else chunk, frames - f)
        sizes.append(c)
        f += c
    return sizes


def one_stream(eng, x, sizes):
    """The one-utterance stream (pe_stream_begin / pe_stream_next) of listener x asking for the given chunk sizes, then to
    its end for the last one: [(float, int16)], and the frame count. The sizes are what a caller ASKS for -- the short first
    chunk, then the chunk size -- not what the last, partial chunk delivers: the request sizes the window bucket, and with
    it the kernel forms, so only equal requests give equal bits."""
    lib, h = eng._lib, eng._h
    ids = np.ascontiguousarray(x.ids, np.int64)
    sc = (C.c_float * 3)(*x.scales)
    keep = []
    nref = eng._noise(x.nw[None], x.nz[None], keep)
    frames, halo = C.c_int32(), C.c_int32()
    eng._check(lib.pe_stream_begin(h, ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size, sc, -1 if x.sid is None else int(x.sid),
                                   nref, C.byref(frames), C.byref(halo)))
    out, k = [], 0
    while True:
        a, p, n = C.POINTER(C.c_float)(), C.POINTER(C.c_int16)(), C.c_int64()
        eng._check(lib.pe_stream_next(h, int(sizes[min(k, len(sizes) - 1)]), C.byref(a), C.byref(p), C.byref(n)))
        if n.value == 0:
            return out, frames.value
        out.append((np.ctypeslib.as_array(a, (n.value,)).copy(), np.ctypeslib.as_array(p, (n.value,)).copy()))
        k += 1


def oracle_chunks(O, wt, cfg, z, sizes, halo, sid):
    """oracle.stream_chunks for chunk sizes that differ from chunk to chunk: the same cut, padding, trim and int16 rule,
    statement by statement (stream_chunks takes one size for the whole utterance; a listener that joins a pool takes a short
    first chunk). For equal sizes the callers check that it IS stream_chunks, bit for bit."""
    import torch
    import torch.nn.functional as F
    zt = torch.as_tensor(np.asarray(z), dtype=wt["enc_p.emb.weight"].dtype)[None]
    g = None
    if cfg.n_speakers > 1:
        g = F.embedding(torch.tensor([int(sid or 0)]), wt["emb_g.weight"]).unsqueeze(-1)
    Fr = zt.shape[2]
    hop = int(np.prod(cfg.up_rates))
    out, s = [], 0
    with torch.no_grad():
        for c in sizes:
            e = min(Fr, s + c)
            ps, pe = min(halo, s), min(halo, Fr - e)
            a = O.generator(wt, cfg, zt[:, :, s - ps:e + pe], g=g)[0, 0].numpy()
            a = a[ps * hop:a.size - pe * hop]
            out.append((a, O.audio_float_to_int16(a)))
            s = e
    return out


def pcm_rms(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)) / 32767.0
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def check(eng, cfg, w, texts, chunk, first, halo, one_tol, oracle_tol, rms_tol):
    """Every listener against its references; returns the worst figures. No listener is left out: the one that left is
    compared on the chunks it received."""
    from oracle import vits_oracle as O
    wt = O.to_torch(w)
    worst = dict(one=0.0, oracle=0.0, rms=0.0)
    assert sum(1 for x in texts if x.left) == 1
    for i, x in enumerate(texts):
        want = expected_sizes(x.frames, 0 if i == 2 else first, chunk)
        if x.left:
            assert 0 < len(x.sizes) < len(want) and x.sizes == want[:len(x.sizes)], (x.name, x.sizes, want)
        else:
            assert x.sizes == want, (x.name, x.sizes, want)           # the number of chunks it has alone
        one, f1 = one_stream(eng, x, ([] if i == 2 else [first]) + [chunk])
        assert f1 == x.frames and len(one) == len(want), x.name
        o = O.synthesize(wt, cfg, x.ids, x.scales, x.nw, x.nz, sid=x.sid, keep=True)
        assert int(o["frames"]) == x.frames, (x.name, x.frames, o["frames"])
        ref = oracle_chunks(O, wt, cfg, o["z"], want, halo, x.sid)
        if i == 2:
            # equal sizes: the restatement above is oracle.stream_chunks, and the schedule-driven one-utterance stream is
            # Engine.stream
            direct = O.stream_chunks(wt, cfg, o["z"], chunk, halo, sid=x.sid)
            assert len(direct) == len(ref)
            assert all(np.array_equal(a, b) and np.array_equal(p, q) for (a, p), (b, q) in zip(direct, ref))
            es = list(eng.stream(x.ids, x.scales, sid=x.sid, chunk_frames=chunk, noise_w=x.nw, noise_z=x.nz))
            assert len(es) == len(one)
            assert all(np.array_equal(a, b) and np.array_equal(p, q) for (a, p), (b, q) in zip(es, one))
        for k, ((a, p), (a1, p1), (ra, rp)) in enumerate(zip(x.chunks, one, ref)):
            assert a.shape == a1.shape == ra.shape and p.shape == rp.shape, (x.name, k)
            assert p.dtype == np.int16 and np.array_equal(O.audio_float_to_int16(a), p), (x.name, k)
            worst["one"] = max(worst["one"], float(np.max(np.abs(a - a1))))
            worst["oracle"] = max(worst["oracle"], float(np.max(np.abs(a - ra))))
            worst["rms"] = max(worst["rms"], pcm_rms(p, rp))
            assert np.max(np.abs(a - a1)) < one_tol, (x.name, k, worst)
            assert np.max(np.abs(a - ra)) < oracle_tol, (x.name, k, worst)
            assert pcm_rms(p, rp) <= rms_tol, (x.name, k, worst)
    return worst


def digest(texts):
    h = hashlib.sha256()
    for x in texts:
        for _, p in x.chunks:
            h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


# ---- the emulator's inputs: tests/emu/stream_batch_case.py's three texts and a fourth, 14 ids from another seed
CHUNK, FIRST = 4, 2
FOURTH_SID = 2


def emu_texts(cfg, multi_speaker):
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import stream_batch_case as K
    ids, nw, nz = K.inputs(cfg)
    scales = K.SCALES_MS if multi_speaker else K.SCALES
    sids = list(K.SIDS) if multi_speaker else [None] * 3
    texts = [Listener("ids%d" % len(ids[i]), ids[i], scales[i], sids[i], nw[i], nz[i]) for i in range(3)]
    rng = np.random.default_rng(57)
    ids4 = W.synthetic_phoneme_ids(14, 77, id_max=cfg.n_vocab - 1)
    assert not np.array_equal(ids4, ids[1])
    texts.append(Listener("fourth", ids4, scales[1], FOURTH_SID if multi_speaker else None,
                          rng.standard_normal((2, 14)).astype(np.float32),
                          rng.standard_normal((cfg.inter, 48 * 14 + 64)).astype(np.float32)))
    return texts


# ---- the GPU's inputs: the CASES of tests/test_gpu_stream_batch.py. Roles by length: the shortest is text 0, the longest
# text 2, the second shortest joins late (text 3), all others join with text 0.
def gpu_texts(cfg, preset, scales, prior_noise=True):
    import test_gpu_stream_batch as G
    lens, chunk = G.CASES[preset]
    ids, nw, nz = G.inputs_for(cfg, lens)
    order = [0, 2, len(lens) - 1, 1] + list(range(3, len(lens) - 1))
    texts = [Listener("ids%d" % lens[i], ids[i], scales, None, nw[i], nz[i] if prior_noise else None) for i in order]
    return texts, chunk, max(1, chunk // 3)


def gpu_case(preset, one_tol, oracle_tol, rms_tol, scales):
    """The scenario on the GPU, every delivered chunk against the one-utterance stream and the oracle; the frame counts
    agree with the oracle's under the guard of tests/test_gpu_stream_batch.py: no duration within 1e-4 of an integer
    before the ceil (five times the distance at which another summation order can flip a frame)."""
    from oracle import vits_oracle as O
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), device=0)
    texts, chunk, first = gpu_texts(cfg, preset, scales)
    wt = O.to_torch(w)
    dist = 1.0
    for x in texts:
        _, wv = O.durations_only(wt, cfg, x.ids, x.scales, x.nw, return_w=True)
        dist = min(dist, float(np.min(np.abs(wv - np.round(wv)))))
    print(f"\n[{preset}] smallest distance of a pre-ceil duration from an integer: {dist:.3g}")
    assert dist >= 1e-4, dist
    pool = play(eng, texts, chunk, first, max_frames=512)
    halo = pool.halo
    worst = check(eng, cfg, w, texts, chunk, first, halo, one_tol, oracle_tol, rms_tol)
    pool.close()
    eng.close()
    worst.update(frames=[x.frames for x in texts], chunks=[len(x.chunks) for x in texts], halo=halo,
                 left=[x.name for x in texts if x.left], reused_slot=texts[3].slot)
    return worst


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--gpu":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import test_gpu_stream_batch as G
        print(json.dumps(gpu_case(sys.argv[2], G.CHUNK_TOL, G.TIGHT_AUDIO_TOL, G.RMS_TOL, G.SCALES)))
        return
    elib = L.bind(os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so"))
    cfg = W.preset("tiny-ms")
    w = W.synthetic_weights(cfg, 1234)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=elib)
    texts = emu_texts(cfg, True)
    play(eng, texts, CHUNK, FIRST).close()
    print(json.dumps({"order": os.environ.get("EMU_ORDER", ""), "sizes": [x.sizes for x in texts],
                      "frames": [x.frames for x in texts], "pcm_sha256": digest(texts)}))
    eng.close()


if __name__ == "__main__":
    main()
