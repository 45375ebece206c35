"""Python handle on the HIP engine (C ABI in include/piper_hip.h).

This is the host-side twin of what ``onnxruntime.InferenceSession`` is to the reference's
``PiperVoice`` (reference src/python_run/piper/voice.py:24-55,140-185): ``run()`` takes the same
feed (``input``, ``scales``, optional ``sid``) and returns the float waveform; everything is
computed on the GPU by libpiper_hip.so.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _lib as L


class EngineError(RuntimeError):
    pass


class Synthesis:
    """Result of one (batched) synthesis call. Arrays are copies (the C side reuses its buffers)."""

    def __init__(self, audio: List[np.ndarray], pcm: List[np.ndarray], frames: np.ndarray, infer_seconds: float, codes=None):
        self.audio = audio
        self.pcm = pcm
        self.frames = frames
        self.infer_seconds = infer_seconds
        self.codes = codes          # G.711 codes, one uint8 array per utterance; None with the sample format "s16"


class Chunk(tuple):
    """One row of a stream chunk: the ``(float chunk or None, int16 chunk)`` pair it always was, with ``codes`` -- the
    chunk's G.711 codes as a uint8 array, None with the sample format "s16"."""

    def __new__(cls, audio, pcm, codes=None):
        t = super().__new__(cls, (audio, pcm))
        t.codes = codes
        return t

    audio = property(lambda self: self[0])
    pcm = property(lambda self: self[1])


def per_utterance_scales(scales, batch: int):
    """None for one (noise_scale, length_scale, noise_w) triple (the call's scales); a C-contiguous float32 [batch][3] array
    for one triple per utterance (the *_scaled entry points of include/piper_hip.h)."""
    a = np.asarray(scales, dtype=np.float32)
    if a.shape == (3,):
        return None
    if a.shape != (batch, 3):
        raise ValueError(f"scales must be one triple or a ({batch}, 3) array, got shape {a.shape}")
    return np.ascontiguousarray(a)


class Timing:
    """A timing plan (include/piper_hip.h: pe_timing) as per-utterance lists. ``rate``: one array of per-id multipliers of
    the predicted durations per utterance (an entry None: all 1). ``durations``: one int array per utterance, >= 0 = that id
    lasts exactly so many frames, -1 = predicted (an entry None: all predicted). ``target_frames``: one int per utterance,
    0 = no target. Any of the three may be None."""

    def __init__(self, rate=None, durations=None, target_frames=None):
        self.rate, self.durations, self.target_frames = rate, durations, target_frames

    def pack(self, id_lists, keep: list):
        """The C struct for ``id_lists`` (by reference); the arrays it points to are appended to ``keep``."""
        lens = [len(s) for s in id_lists]
        t = L.PeTiming()

        def rows(per, dtype, fill, what):
            if len(per) != len(lens):
                raise ValueError(f"{what}: {len(per)} entries for {len(lens)} utterances")
            out = []
            for b, (r, n) in enumerate(zip(per, lens)):
                a = np.full(n, fill, dtype) if r is None else np.asarray(r, dtype).reshape(-1)
                if a.size != n:
                    raise ValueError(f"{what} of utterance {b}: {a.size} values for {n} ids")
                out.append(a)
            return np.ascontiguousarray(np.concatenate(out)) if out else np.zeros(0, dtype)

        if self.rate is not None:
            a = rows(self.rate, np.float32, 1.0, "rate")
            keep.append(a)
            t.rate = a.ctypes.data_as(C.POINTER(C.c_float))
        if self.durations is not None:
            a = rows(self.durations, np.int32, -1, "durations")
            keep.append(a)
            t.forced = a.ctypes.data_as(C.POINTER(C.c_int32))
        if self.target_frames is not None:
            a = np.ascontiguousarray(self.target_frames, np.int32).reshape(-1)
            if a.size != len(lens):
                raise ValueError(f"target_frames: {a.size} entries for {len(lens)} utterances")
            keep.append(a)
            t.target_frames = a.ctypes.data_as(C.POINTER(C.c_int32))
        keep.append(t)
        return C.byref(t)


def pack_seeds(seeds, batch: int, keep: list):
    """The C struct (by reference) for per-utterance noise seeds (include/piper_hip.h: pe_seeds), or None for ``seeds`` None.
    ``seeds``: one entry per utterance, an int (any value, taken modulo 2^64) or None for an utterance that draws from the
    engine's own stream. The arrays it points to are appended to ``keep``."""
    if seeds is None:
        return None
    seeds = list(seeds)
    if len(seeds) != batch:
        raise ValueError(f"seeds: {len(seeds)} entries for {batch} utterances")
    val = np.array([0 if s is None else int(s) % (1 << 64) for s in seeds], np.uint64).reshape(-1)
    use = np.array([0 if s is None else 1 for s in seeds], np.uint8).reshape(-1)
    val, use = np.ascontiguousarray(val), np.ascontiguousarray(use)
    s = L.PeSeeds()
    s.seed = val.ctypes.data_as(C.POINTER(C.c_uint64))
    s.use = use.ctypes.data_as(C.POINTER(C.c_uint8))
    keep.extend([val, use, s])
    return C.byref(s)


def pack_speakers(speakers, sids, batch: int, gin: int, keep: list):
    """-> (sids, blend): the plain speaker ids of a call and the C struct (by reference) of its speaker blends
    (include/piper_hip.h: pe_blend), or ``(sids, None)`` as given when no utterance carries a blend or a vector.
    ``speakers``: one entry per utterance -- None or an int, a plain id like ``sids``; a mapping ``{sid: weight}`` or a
    sequence of ``(sid, weight)`` pairs, a blend whose components keep their order (a dict's insertion order); a 1-D float
    array of ``gin`` values, a speaker vector. An utterance may not have both a ``sids`` entry and a ``speakers`` entry."""
    if speakers is None:
        return sids, None
    speakers = list(speakers)
    if len(speakers) != batch:
        raise ValueError(f"speakers: {len(speakers)} entries for {batch} utterances")
    if sids is not None and len(sids) != batch:
        raise ValueError(f"sids: {len(sids)} entries for {batch} utterances")
    plain = [0] * batch
    count = np.zeros(batch, np.int32)
    comp_s, comp_w = [], []
    vec = None
    for b, sp in enumerate(speakers):
        given = sids is not None and sids[b] is not None
        if sp is None:
            plain[b] = int(sids[b]) if given else 0
            continue
        if given:
            raise ValueError(f"utterance {b}: both sids and speakers are given")
        if isinstance(sp, (int, np.integer)):
            plain[b] = int(sp)
            continue
        if isinstance(sp, dict):
            pairs = list(sp.items())
        elif isinstance(sp, np.ndarray) or (len(sp) > 0 and not isinstance(sp[0], (tuple, list))):
            v = np.asarray(sp, np.float32)
            if v.ndim != 1 or v.size != gin:
                raise ValueError(f"utterance {b}: a speaker vector has {gin} values (1-D), got shape {v.shape}")
            if vec is None:
                vec = np.zeros((batch, max(gin, 1)), np.float32)
            vec[b, :gin] = v
            count[b] = -1
            continue
        else:
            pairs = [tuple(q) for q in sp]
        if len(pairs) == 0:
            raise ValueError(f"utterance {b}: an empty speaker blend")
        count[b] = len(pairs)
        comp_s += [int(q[0]) for q in pairs]
        comp_w += [float(q[1]) for q in pairs]
    if not count.any():
        return (None if sids is None and not any(plain) else plain), None
    bs = np.ascontiguousarray(comp_s, np.int64).reshape(-1)
    bw = np.ascontiguousarray(comp_w, np.float32).reshape(-1)
    bl = L.PeBlend()
    bl.count = count.ctypes.data_as(C.POINTER(C.c_int32))
    if bs.size:
        bl.sid = bs.ctypes.data_as(C.POINTER(C.c_int64))
        bl.weight = bw.ctypes.data_as(C.POINTER(C.c_float))
    if vec is not None:
        bl.vector = vec.ctypes.data_as(C.POINTER(C.c_float))
    keep.extend([count, bs, bw, vec, bl])
    return plain, C.byref(bl)


def _tiled_scales(scales, batch: int):
    per = per_utterance_scales(scales, batch)
    if per is None:
        per = np.ascontiguousarray(np.tile(np.asarray(scales, np.float32), (max(batch, 1), 1)))
    return per


class Engine:
    def __init__(self, *, onnx_path: Optional[str] = None, blob: Optional[bytes] = None, device: int = 0,
                 lib: Optional[C.CDLL] = None, arena=None, skeleton: bool = False):
        """``arena`` = (device pointer, bytes) of a caller-owned weight arena (multi-GPU loading: see
        piper_amd.dist.load_sharded); with ``skeleton`` the blob may be just the header of a PEBLOB01 and the arena's
        content is expected to arrive by broadcast before ``arena_ready()``."""
        self._lib = lib if lib is not None else L.get_lib()
        self._h = C.c_void_p()
        if (onnx_path is None) == (blob is None):
            raise ValueError("give exactly one of onnx_path / blob")
        if onnx_path is not None:
            rc = self._lib.pe_create(str(onnx_path).encode(), device, C.byref(self._h))
        elif arena is not None:
            self._blob = bytes(blob)
            rc = self._lib.pe_create_in_arena(self._blob, len(self._blob), device, C.c_void_p(int(arena[0])), int(arena[1]),
                                              int(bool(skeleton)), C.byref(self._h))
        else:
            self._blob = bytes(blob)
            rc = self._lib.pe_create_from_blob(self._blob, len(self._blob), device, C.byref(self._h))
        self._check(rc)
        sr, hop, nspk, nsym, wb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self._lib.pe_get_info(self._h, C.byref(sr), C.byref(hop), C.byref(nspk), C.byref(nsym),
                                          C.byref(wb)))
        self.sample_rate, self.hop, self.num_speakers, self.num_symbols = sr.value, hop.value, nspk.value, nsym.value
        self.weight_bytes = wb.value
        self.speaker_dim = self._speaker_dim()

    def _speaker_dim(self) -> int:
        gin = C.c_int32()
        self._check(self._lib.pe_get_speaker_dim(self._h, C.byref(gin)))
        return gin.value

    def speaker_embedding(self, sid: int) -> np.ndarray:
        """Row ``sid`` of the voice's speaker table, ``speaker_dim`` float32 values (pe_get_speaker_embedding): for callers
        who do their own arithmetic and come back with a vector (``speakers=[vector]``)."""
        out = np.zeros(max(self.speaker_dim, 1), np.float32)
        self._check(self._lib.pe_get_speaker_embedding(self._h, int(sid), out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out[:self.speaker_dim]

    def debug_blend(self, speakers, sids=None) -> np.ndarray:
        """Test hook (pe_debug_blend): the speaker vectors ``[batch][speaker_dim]`` the mixing kernel forms for ``speakers``
        (as in ``synthesize_batch``), no synthesis."""
        keep: list = []
        n = len(speakers)
        plain, bl = pack_speakers(speakers, sids, n, self.speaker_dim, keep)
        if bl is None:
            count = np.zeros(n, np.int32)
            b = L.PeBlend()
            b.count = count.ctypes.data_as(C.POINTER(C.c_int32))
            keep.extend([count, b])
            bl = C.byref(b)
        sid_np = None if plain is None else np.ascontiguousarray(plain, np.int64)
        out = np.zeros((n, self.speaker_dim), np.float32)
        self._check(self._lib.pe_debug_blend(self._h, bl, n, None if sid_np is None else sid_np.ctypes.data_as(C.POINTER(C.c_int64)),
                                             out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    @classmethod
    def borrowed(cls, lib: C.CDLL, handle: int) -> "Engine":
        """View of an engine somebody else owns (``pe_group_engine``): every method works, ``close()`` does not destroy."""
        self = cls.__new__(cls)
        self._lib, self._h, self._borrowed = lib, C.c_void_p(int(handle)), True
        sr, hop, nspk, nsym, wb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
        self._check(lib.pe_get_info(self._h, C.byref(sr), C.byref(hop), C.byref(nspk), C.byref(nsym), C.byref(wb)))
        self.sample_rate, self.hop, self.num_speakers, self.num_symbols = sr.value, hop.value, nspk.value, nsym.value
        self.weight_bytes = wb.value
        self.speaker_dim = self._speaker_dim()
        return self

    def weights_used(self) -> int:
        n = C.c_size_t()
        self._check(self._lib.pe_weights_used(self._h, C.byref(n)))
        return int(n.value)

    def arena_ready(self):
        self._check(self._lib.pe_arena_ready(self._h))

    def _check(self, rc: int):
        if rc != 0:
            raise EngineError(self._lib.pe_last_error().decode(errors="replace"))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            if not getattr(self, "_borrowed", False):
                self._lib.pe_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    @staticmethod
    def _pack(id_lists: Sequence[Sequence[int]]):
        offs = np.zeros(len(id_lists) + 1, np.int64)
        for i, s in enumerate(id_lists):
            offs[i + 1] = offs[i] + len(s)
        ids = np.concatenate([np.asarray(s, np.int64).reshape(-1) for s in id_lists]) if id_lists else \
            np.zeros(0, np.int64)
        return np.ascontiguousarray(ids), offs

    def _noise(self, noise_w, noise_z, keep):
        if noise_w is None and noise_z is None:
            return None
        n = L.PeNoise()
        if noise_w is not None:
            a = np.ascontiguousarray(noise_w, np.float32)      # [B][2][stride]
            keep.append(a)
            n.noise_w = a.ctypes.data_as(C.POINTER(C.c_float))
            n.w_stride = a.shape[-1]
        if noise_z is not None:
            a = np.ascontiguousarray(noise_z, np.float32)      # [B][inter][stride]
            keep.append(a)
            n.noise_z = a.ctypes.data_as(C.POINTER(C.c_float))
            n.z_stride = a.shape[-1]
        keep.append(n)
        return C.byref(n)

    def _collect(self, res: L.PeResult, want_audio=True, want_pcm=True) -> Synthesis:
        B = res.batch
        offs = np.frombuffer(C.string_at(res.sample_offsets, 8 * (B + 1)), np.int64)
        frames = np.frombuffer(C.string_at(res.frames, 4 * B), np.int32).copy()
        total = int(offs[-1])
        audio, pcm = [], []
        # (one copy out of the engine's pinned buffers through string_at; np.ctypeslib.as_array would build a new ctypes
        # array type for every distinct sample count -- ~0.7 ms per call when the frame counts change from call to call)
        if want_audio and total:
            a = np.frombuffer(bytearray(C.string_at(res.audio, 4 * total)), np.float32)
            audio = [a[offs[i]:offs[i + 1]] for i in range(B)]
        if want_pcm and total:
            p = np.frombuffer(bytearray(C.string_at(res.pcm, 2 * total)), np.int16)
            pcm = [p[offs[i]:offs[i + 1]] for i in range(B)]
        return Synthesis(audio, pcm, frames, res.infer_seconds, self._last_codes(0))

    def _last_codes(self, which: int):
        """pe_last_codes as a list of uint8 arrays, one per row; None when that call ran with the format "s16"."""
        cp, op, rows = C.POINTER(C.c_uint8)(), C.POINTER(C.c_int64)(), C.c_int32()
        self._check(self._lib.pe_last_codes(self._h, int(which), C.byref(cp), C.byref(op), C.byref(rows)))
        if rows.value == 0:
            return None
        offs = np.frombuffer(C.string_at(op, 8 * (rows.value + 1)), np.int64)
        total = int(offs[-1])
        c = np.frombuffer(bytearray(C.string_at(cp, total)) if total else bytearray(), np.uint8)
        return [c[offs[i]:offs[i + 1]] for i in range(rows.value)]

    # ---- API
    def synthesize_batch(self, id_lists, scales=(0.667, 1.0, 0.8), sids=None, noise_w=None, noise_z=None,
                         timing: Optional[Timing] = None, seeds=None, speakers=None) -> Synthesis:
        """``scales``: one (noise_scale, length_scale, noise_w) triple for every utterance, or a (B, 3) array with one
        triple per utterance (pe_synthesize_batch_scaled). ``timing``: a ``Timing`` plan (pe_synthesize_batch_timed).
        ``seeds``: one int or None per utterance (pe_synthesize_batch_seeded): a seeded utterance's noise, and with it its
        audio, depends on its seed alone -- not on the handle, the calls before or the rest of the batch.
        ``speakers``: one entry per utterance (pe_synthesize_batch_blended) -- None or an int, a plain id; ``{sid: weight}`` or
        ``(sid, weight)`` pairs, a blend of table rows in that order; a 1-D array of ``speaker_dim`` floats, a vector."""
        ids, offs = self._pack(id_lists)
        keep0: list = []
        sids, blend = pack_speakers(speakers, sids, len(id_lists), self.speaker_dim, keep0)
        plain = timing is None and seeds is None and blend is None
        per = per_utterance_scales(scales, len(id_lists)) if plain else _tiled_scales(scales, len(id_lists))
        sc = (C.c_float * 3)(*[float(s) for s in scales]) if per is None else per.ctypes.data_as(C.POINTER(C.c_float))
        entry = self._lib.pe_synthesize_batch if per is None else self._lib.pe_synthesize_batch_scaled
        keep: list = [per]
        extra = ()
        if timing is not None:
            entry, extra = self._lib.pe_synthesize_batch_timed, (timing.pack(id_lists, keep),)
        if seeds is not None:
            entry, extra = self._lib.pe_synthesize_batch_seeded, (extra[0] if extra else None, pack_seeds(seeds, len(id_lists), keep))
        if blend is not None:
            keep += keep0
            entry, extra = self._lib.pe_synthesize_batch_blended, ((extra + (None, None))[0], (extra + (None, None))[1], blend)
        nz = self._noise(noise_w, noise_z, keep)
        sid_arr = None
        if sids is not None:
            sid_np = np.ascontiguousarray(sids, np.int64)
            keep.append(sid_np)
            sid_arr = sid_np.ctypes.data_as(C.POINTER(C.c_int64))
        res = L.PeResult()
        self._check(entry(
            self._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), offs.ctypes.data_as(C.POINTER(C.c_int64)),
            len(id_lists), sc, sid_arr, nz, C.byref(res), *extra))
        return self._collect(res)

    def synthesize(self, ids, scales=(0.667, 1.0, 0.8), sid=None, noise_w=None, noise_z=None, seed=None,
                   speaker=None) -> Synthesis:
        nw = None if noise_w is None else np.asarray(noise_w, np.float32)[None]
        nz = None if noise_z is None else np.asarray(noise_z, np.float32)[None]
        return self.synthesize_batch([ids], scales, None if sid is None else [sid], nw, nz,
                                     seeds=None if seed is None else [seed],
                                     speakers=None if speaker is None else [speaker])

    def upload(self, id_lists, scales=(0.667, 1.0, 0.8), sids=None, noise_w=None, noise_z=None,
               timing: Optional[Timing] = None, seeds=None, speakers=None):
        """``scales``: one triple, or a (B, 3) array of per-utterance triples (pe_upload_scaled). ``timing``: a ``Timing``
        plan (pe_upload_timed); every ``run()`` on the upload follows it. ``seeds``: one int or None per utterance
        (pe_upload_seeded); every ``run()`` on the upload draws the same noise again. ``speakers`` as in
        ``synthesize_batch`` (pe_upload_blended); every ``run()`` on the upload keeps the blend."""
        ids, offs = self._pack(id_lists)
        keep0: list = []
        sids, blend = pack_speakers(speakers, sids, len(id_lists), self.speaker_dim, keep0)
        plain = timing is None and seeds is None and blend is None
        per = per_utterance_scales(scales, len(id_lists)) if plain else _tiled_scales(scales, len(id_lists))
        sc = (C.c_float * 3)(*[float(s) for s in scales]) if per is None else per.ctypes.data_as(C.POINTER(C.c_float))
        entry = self._lib.pe_upload if per is None else self._lib.pe_upload_scaled
        keep: list = [per]
        extra = ()
        if timing is not None:
            entry, extra = self._lib.pe_upload_timed, (timing.pack(id_lists, keep),)
        if seeds is not None:
            entry, extra = self._lib.pe_upload_seeded, (extra[0] if extra else None, pack_seeds(seeds, len(id_lists), keep))
        if blend is not None:
            keep += keep0
            entry, extra = self._lib.pe_upload_blended, ((extra + (None, None))[0], (extra + (None, None))[1], blend)
        nz = self._noise(noise_w, noise_z, keep)
        sid_arr = None
        if sids is not None:
            sid_np = np.ascontiguousarray(sids, np.int64)
            keep.append(sid_np)
            sid_arr = sid_np.ctypes.data_as(C.POINTER(C.c_int64))
        self._keep = keep          # noise_z is read during run()
        self._check(entry(self._h, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                          offs.ctypes.data_as(C.POINTER(C.c_int64)), len(id_lists), sc, sid_arr, nz, *extra))

    def pack_host(self, id_lists, scales=(0.667, 1.0, 0.8), timing: Optional[Timing] = None):
        """The host-side inputs of a call as the C ABI takes them -- int64 ids, prefix offsets, float scales in host
        memory, what piper::synthesize wraps as Ort tensors (reference piper.cpp:342-365) -- built once, for callers that
        time whole calls (bench.py) without Python's list handling inside the timed region. With ``timing`` the plan is
        packed as well and ``upload_host`` goes through pe_upload_timed."""
        ids, offs = self._pack(id_lists)
        if timing is not None:
            per = _tiled_scales(scales, len(id_lists))
            keep: list = [per]
            tref = timing.pack(id_lists, keep)
            return (ids, offs, per.ctypes.data_as(C.POINTER(C.c_float)), ids.ctypes.data_as(C.POINTER(C.c_int64)),
                    offs.ctypes.data_as(C.POINTER(C.c_int64)), len(id_lists), tref, keep)
        sc = (C.c_float * 3)(*[float(s) for s in scales])
        return (ids, offs, sc, ids.ctypes.data_as(C.POINTER(C.c_int64)), offs.ctypes.data_as(C.POINTER(C.c_int64)),
                len(id_lists))

    def upload_host(self, packed):
        """pe_upload of inputs prepared by pack_host: host ids -> device, the engine draws both noise sites."""
        self._keep = []
        if len(packed) > 6:
            self._check(self._lib.pe_upload_timed(self._h, packed[3], packed[4], packed[5], packed[2], None, None, packed[6]))
            return
        self._check(self._lib.pe_upload(self._h, packed[3], packed[4], packed[5], packed[2], None, None))

    def run(self):
        self._check(self._lib.pe_run(self._h))

    def fetch(self, want_audio=True, want_pcm=True) -> Synthesis:
        res = L.PeResult()
        self._check(self._lib.pe_fetch(self._h, int(want_audio), int(want_pcm), C.byref(res)))
        return self._collect(res, want_audio, want_pcm)

    def fetch_views(self, want_audio=True, want_pcm=True) -> "L.PeResult":
        """Like fetch() but returns the C ABI's result views as they are (pointers into the engine's pinned host
        buffers, valid until the next call) -- what a C / C++ caller gets; no numpy copies."""
        res = L.PeResult()
        self._check(self._lib.pe_fetch(self._h, int(want_audio), int(want_pcm), C.byref(res)))
        return res

    def stream(self, ids, scales=(0.667, 1.0, 0.8), sid=None, chunk_frames: int = 45, noise_w=None, noise_z=None, seed=None,
               speaker=None, codes: bool = False):
        """Generator over (float_audio, int16_pcm) chunks of one utterance: encoder/flow once, then the
        vocoder on exact-halo windows of `chunk_frames` frames (reference default 45). Concatenating
        the float chunks gives exactly the unchunked waveform; pcm is peak-normalised per chunk, or follows
        the level set by ``set_stream_gain``. ``seed``: the utterance's noise seed (pe_stream_begin_seeded). ``speaker``: the utterance's
        entry of ``speakers`` as in ``synthesize_batch`` (pe_stream_begin_blended). ``codes`` True: triples
        (float_audio, int16_pcm, uint8 G.711 codes or None), the codes of ``set_sample_format``."""
        ids_np = np.ascontiguousarray(ids, np.int64)
        sc = (C.c_float * 3)(*[float(s) for s in scales])
        keep: list = []
        nw = None if noise_w is None else np.asarray(noise_w, np.float32)[None]
        nz = None if noise_z is None else np.asarray(noise_z, np.float32)[None]
        nref = self._noise(nw, nz, keep)
        frames, halo = C.c_int32(), C.c_int32()
        entry, extra = self._lib.pe_stream_begin, ()
        if seed is not None:
            entry, extra = self._lib.pe_stream_begin_seeded, (None, pack_seeds([seed], 1, keep))
        if speaker is not None:
            one, blend = pack_speakers([speaker], None if sid is None else [sid], 1, self.speaker_dim, keep)
            sid = None if one is None else one[0]
            if blend is not None:
                entry, extra = self._lib.pe_stream_begin_blended, (None, extra[1] if extra else None, blend)
        self._check(entry(self._h, ids_np.ctypes.data_as(C.POINTER(C.c_int64)), ids_np.size, sc,
                          -1 if sid is None else int(sid), nref, C.byref(frames), C.byref(halo), *extra))
        self.stream_frames, self.stream_halo = frames.value, halo.value
        done = 0
        while True:
            a, p, n = C.POINTER(C.c_float)(), C.POINTER(C.c_int16)(), C.c_int64()
            self._check(self._lib.pe_stream_next(self._h, int(chunk_frames), C.byref(a), C.byref(p), C.byref(n)))
            if n.value == 0:
                # (the end is decided by the frames: with the stream limiter a call may hand out nothing and go on)
                if done >= frames.value:
                    return
                done = min(frames.value, done + int(chunk_frames))
                if codes:
                    yield (np.zeros(0, np.float32), np.zeros(0, np.int16),
                           None if self.sample_format == "s16" else np.zeros(0, np.uint8))
                else:
                    yield np.zeros(0, np.float32), np.zeros(0, np.int16)
                continue
            done = min(frames.value, done + int(chunk_frames))
            pair = (np.ctypeslib.as_array(a, (n.value,)).copy(), np.ctypeslib.as_array(p, (n.value,)).copy())
            if codes:
                c = self._last_codes(1)
                yield pair + (None if c is None else c[0],)
            else:
                yield pair

    def stream_batch(self, id_lists, scales=(0.667, 1.0, 0.8), sids=None, chunk_frames=45, noise_w=None, noise_z=None,
                     want_audio: bool = True, timing: Optional[Timing] = None, seeds=None, speakers=None):
        """Generator over the chunks of B utterances streamed in lock step (pe_stream_begin_batch / pe_stream_next_batch):
        text encoder, durations and flow for the whole batch once, then one batched vocoder pass per chunk. Every item
        is a list of B ``(float chunk or None, int16 chunk)`` pairs -- empty arrays for utterances that are finished;
        chunk k of utterance b is what ``stream`` yields for that utterance alone, in every ``set_stream_gain`` mode (each
        utterance carries its own level). ``chunk_frames``: an int, or a
        callable ``k -> frames`` of the chunk index (a short first chunk, longer ones after). ``scales``, ``timing`` and
        ``seeds`` and ``speakers`` as in ``synthesize_batch``. Sets ``stream_frames`` (array of B) and ``stream_halo``."""
        B = len(id_lists)
        ids, offs = self._pack(id_lists)
        per = per_utterance_scales(scales, B)
        if per is None:
            per = np.ascontiguousarray(np.tile(np.asarray(scales, np.float32), (B, 1)))
        keep: list = [per]
        sids, blend = pack_speakers(speakers, sids, B, self.speaker_dim, keep)
        nref = self._noise(noise_w, noise_z, keep)
        sid_arr = None
        if sids is not None:
            sid_np = np.ascontiguousarray(sids, np.int64)
            keep.append(sid_np)
            sid_arr = sid_np.ctypes.data_as(C.POINTER(C.c_int64))
        frames, halo = np.zeros(max(B, 1), np.int32), C.c_int32()
        entry, extra = self._lib.pe_stream_begin_batch, ()
        if timing is not None:
            entry, extra = self._lib.pe_stream_begin_batch_timed, (timing.pack(id_lists, keep),)
        if seeds is not None:
            entry, extra = self._lib.pe_stream_begin_batch_seeded, (extra[0] if extra else None, pack_seeds(seeds, B, keep))
        if blend is not None:
            entry, extra = self._lib.pe_stream_begin_batch_blended, ((extra + (None, None))[0], (extra + (None, None))[1], blend)
        self._check(entry(
            self._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), offs.ctypes.data_as(C.POINTER(C.c_int64)), B,
            per.ctypes.data_as(C.POINTER(C.c_float)), sid_arr, nref, frames.ctypes.data_as(C.POINTER(C.c_int32)),
            C.byref(halo), *extra))
        self.stream_frames, self.stream_halo = frames[:B].copy(), halo.value
        self.stream_frames_done = np.zeros(B, np.int32)
        k = 0
        while True:
            cf = int(chunk_frames(k)) if callable(chunk_frames) else int(chunk_frames)
            ch = L.PeStreamChunk()
            before = self.stream_frames_done
            self._check(self._lib.pe_stream_next_batch(self._h, cf, int(bool(want_audio)), C.byref(ch)))
            offs_k = np.frombuffer(C.string_at(ch.sample_offsets, 8 * (B + 1)), np.int64)
            self.stream_frames_done = np.frombuffer(C.string_at(ch.frames_done, 4 * B), np.int32).copy()
            total = int(offs_k[-1])
            if total == 0:
                # (the end is decided by the frames: with the stream limiter a call may hand out nothing and go on)
                if not np.any(before < self.stream_frames):
                    return
                empty = np.zeros(0, np.float32) if want_audio else None
                none = None if self.sample_format == "s16" else np.zeros(0, np.uint8)
                yield [Chunk(empty, np.zeros(0, np.int16), none) for _ in range(B)]
                k += 1
                continue
            p = np.frombuffer(bytearray(C.string_at(ch.pcm, 2 * total)), np.int16)
            a = np.frombuffer(bytearray(C.string_at(ch.audio, 4 * total)), np.float32) if ch.audio else None
            c = self._last_codes(1)
            yield [Chunk(None if a is None else a[offs_k[b]:offs_k[b + 1]], p[offs_k[b]:offs_k[b + 1]],
                         None if c is None else c[b]) for b in range(B)]
            k += 1

    def stream_pool(self, slots: int, max_frames: int) -> "StreamPool":
        """Open a stream pool of ``slots`` listeners with utterances of up to ``max_frames`` frames (pe_stream_pool_open):
        listeners join and leave while others are in mid-stream. Use as a context manager, or ``close()`` it."""
        return StreamPool(self, slots, max_frames)

    def durations(self) -> np.ndarray:
        n = C.c_int64()
        self._check(self._lib.pe_get_durations(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        self._check(self._lib.pe_get_durations(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size,
                                               C.byref(n)))
        return out

    def set_output_rate(self, rate: Optional[int], native: Optional[int] = None):
        """Deliver everything -- whole utterances and stream chunks -- at ``rate`` Hz, resampled on the device before the
        int16 conversion (include/piper_hip.h: pe_set_output_rate). ``native``: the voice's own rate, needed where the
        voice's header carries none (an .onnx: pass ``audio.sample_rate`` of its .onnx.json). ``rate`` None, 0 or the
        native rate: off. Sample counts are then in output samples; ``frames`` stays in native frames."""
        self._check(self._lib.pe_set_output_rate(self._h, int(native or 0), int(rate or 0)))

    SAMPLE_FORMATS = ("s16", "ulaw", "alaw")

    def set_sample_format(self, fmt: Optional[str] = "s16"):
        """Also deliver G.711 codes (include/piper_hip.h: pe_set_sample_format): ``"ulaw"`` or ``"alaw"``, one uint8 code per
        delivered int16 sample, companded on the device -- ``codes`` of every result and chunk. ``"s16"`` or None: off.
        The int16 and the floats are what they are without it."""
        fmt = "s16" if fmt is None else fmt
        if fmt not in self.SAMPLE_FORMATS:
            raise EngineError(f"unknown sample format {fmt!r}: one of {self.SAMPLE_FORMATS}")
        self._check(self._lib.pe_set_sample_format(self._h, self.SAMPLE_FORMATS.index(fmt)))

    @property
    def sample_format(self) -> str:
        f = C.c_int32()
        self._check(self._lib.pe_get_sample_format(self._h, C.byref(f)))
        return self.SAMPLE_FORMATS[f.value]

    def debug_g711(self, fmt: str, rows, flat: bool = False, pad: int = 0, canary: int = 0xA5, slack: int = 64):
        """Test hook (pe_debug_g711): the encoder kernel alone on int16 ``rows`` -- the rows form, or with ``flat`` the flat
        form on the one row. What lies behind a row's end in the staging matrix holds ``pad``. Returns (codes of the packed
        rows, the ``slack`` bytes behind them), the output buffer pre-filled with ``canary``."""
        B = len(rows)
        valid = np.asarray([len(r) for r in rows], np.int32)
        stride = max(1, int(valid.max()) if B else 1)
        x = np.full((B, stride), pad, np.int16)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.int16)
        total = int(valid.sum())
        out = np.full(total + slack, canary, np.uint8)
        self._check(self._lib.pe_debug_g711(self._h, self.SAMPLE_FORMATS.index(fmt), int(bool(flat)),
                                            x.ctypes.data_as(C.POINTER(C.c_int16)), B, stride, valid.ctypes.data_as(C.POINTER(C.c_int32)),
                                            out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out[:total].copy(), out[total:].copy()

    GAIN_MODES = ("chunk", "running", "fixed")

    def set_stream_gain(self, mode: str = "chunk", peak: float = 0.0, ramp_ms: float = 5.0):
        """The int16 level of the chunks of ``stream``, ``stream_batch`` and ``StreamPool`` (include/piper_hip.h:
        pe_set_stream_gain). ``"chunk"``: every chunk normalised by its own peak, the default. ``"fixed"``: every sample
        scaled by ``32767 / max(0.01, peak)``. ``"running"``: one gain per stream that follows the running maximum of the
        chunk peaks (starting at ``peak``; 0 = no prior) and never rises, each change spread over the first ``ramp_ms``
        milliseconds of the chunk that brings it. ``ramp_ms`` is converted to samples with the current ``output_rate``.
        The float chunks are the same in every mode. Not while a stream is live."""
        if mode not in self.GAIN_MODES:
            raise ValueError(f"mode must be one of {self.GAIN_MODES}, got {mode!r}")
        ramp = int(round(float(ramp_ms) * self.output_rate / 1000.0))
        self._check(self._lib.pe_set_stream_gain(self._h, self.GAIN_MODES.index(mode), float(peak), ramp))

    @property
    def stream_gain(self):
        """(mode, peak, ramp in samples) as set by ``set_stream_gain``."""
        m, p, r = C.c_int32(), C.c_float(), C.c_int32()
        self._check(self._lib.pe_get_stream_gain(self._h, C.byref(m), C.byref(p), C.byref(r)))
        return (self.GAIN_MODES + ("loudness",))[m.value], float(p.value), int(r.value)

    def stream_last_gains(self):
        """(gain, peak) float32 arrays of the last chunk call of any kind, one entry per utterance / slot: the gain at the
        chunk's end and the level it came from (pe_stream_last_gains)."""
        n = C.c_int32()
        self._check(self._lib.pe_stream_last_gains(self._h, None, None, 0, C.byref(n)))
        g, p = np.zeros(max(n.value, 1), np.float32), np.zeros(max(n.value, 1), np.float32)
        self._check(self._lib.pe_stream_last_gains(self._h, g.ctypes.data_as(C.POINTER(C.c_float)),
                                                   p.ctypes.data_as(C.POINTER(C.c_float)), g.size, C.byref(n)))
        return g[:n.value], p[:n.value]

    LOUD_SHORT, LOUD_UNMEASURABLE, LOUD_LIMITED = 1, 2, 4
    LOUD_PRIOR = 16

    def set_stream_loudness(self, target_lufs: float, ceiling_db: float = -1.0, prior_lufs=None, ramp_ms: float = 5.0,
                            limiter: bool = False, limiter_ms: float = 5.0):
        """Deliver the chunks of ``stream``, ``stream_batch`` and ``StreamPool`` at a target loudness (include/piper_hip.h:
        pe_set_stream_loudness, stream gain mode ``"loudness"``): every stream carries the running BS.1770-4 gated
        loudness of what it has delivered so far, and each chunk's gain follows it toward ``target_lufs`` under the peak
        ceiling ``ceiling_db``, spread over the chunk's first ``ramp_ms`` milliseconds. ``prior_lufs``: the loudness
        assumed while the stream is too short or too quiet to measure (None: none -- such chunks are delivered as
        generated). The float chunks are the same in every mode. Not while a stream is live; ``set_stream_gain`` leaves
        the mode. ``limiter``: the look-ahead limiter on streams (pe_set_stream_limiter) with a window of ``limiter_ms`` in
        [1, 10] -- a stream whose peaks would have capped its gain keeps the target's gain and only the neighbourhood of the
        peaks is turned down; every stream then holds back ``2 W`` samples (``stream_limiter()``), so a call may hand out
        fewer samples than it generated, or none, and the last call of a stream hands out the rest. A refused call changes
        nothing."""
        ramp = int(round(float(ramp_ms) * self.output_rate / 1000.0))
        prior = float("nan") if prior_lufs is None else float(prior_lufs)
        was = self.stream_limiter()[:2]
        self._check(self._lib.pe_set_stream_limiter(self._h, int(bool(limiter)), float(limiter_ms) if limiter else 0.0))
        if self._lib.pe_set_stream_loudness(self._h, float(target_lufs), float(ceiling_db), prior, ramp):
            err = EngineError(self._lib.pe_last_error().decode(errors="replace"))
            self._lib.pe_set_stream_limiter(self._h, int(was[0]), float(was[1]))
            raise err

    def stream_limiter(self):
        """(on, window_ms, W, D) of the look-ahead limiter on streams (pe_get_stream_limiter): the window and the delay
        ``D = 2 W`` in samples of the delivered rate (0 where the rate is unknown)."""
        on, ms, w, d = C.c_int32(), C.c_float(), C.c_int32(), C.c_int32()
        self._check(self._lib.pe_get_stream_limiter(self._h, C.byref(on), C.byref(ms), C.byref(w), C.byref(d)))
        return bool(on.value), float(ms.value), w.value, d.value

    def stream_last_limiter(self):
        """(max_reduction, shaped_samples) of the last chunk call with the stream limiter, one entry per utterance / slot,
        over the samples that call delivered (pe_stream_last_limiter); empty when it ran without the limiter."""
        n = C.c_int32()
        self._check(self._lib.pe_stream_last_limiter(self._h, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        r, c = np.zeros(m, np.float32), np.zeros(m, np.int32)
        self._check(self._lib.pe_stream_last_limiter(self._h, r.ctypes.data_as(C.POINTER(C.c_float)),
                                                     c.ctypes.data_as(C.POINTER(C.c_int32)), m, C.byref(n)))
        return r[:n.value], c[:n.value]

    @property
    def stream_loudness(self):
        """(on, target_lufs, ceiling_db, prior_lufs or None, ramp in samples) as set by ``set_stream_loudness``."""
        on, t, c, p, r = C.c_int32(), C.c_float(), C.c_float(), C.c_float(), C.c_int32()
        self._check(self._lib.pe_get_stream_loudness(self._h, C.byref(on), C.byref(t), C.byref(c), C.byref(p), C.byref(r)))
        prior = None if p.value != p.value else float(p.value)
        return bool(on.value), float(t.value), float(c.value), prior, int(r.value)

    def stream_last_loudness(self):
        """(lufs, gain, peak, flags) of the last chunk call in the loudness mode, one entry per utterance / slot: the
        running loudness (-inf: not measurable), the gain at the chunk's end, the running peak, LOUD_* bits
        (pe_stream_last_loudness)."""
        n = C.c_int32()
        self._check(self._lib.pe_stream_last_loudness(self._h, None, None, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        L, g, p, f = np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.int32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.pe_stream_last_loudness(self._h, L.ctypes.data_as(fp), g.ctypes.data_as(fp), p.ctypes.data_as(fp),
                                                      f.ctypes.data_as(C.POINTER(C.c_int32)), m, C.byref(n)))
        return L[:n.value], g[:n.value], p[:n.value], f[:n.value]

    PEAK_SAMPLE, PEAK_TRUE = 0, 1

    def set_loudness(self, target_lufs: Optional[float] = None, ceiling_db: float = -1.0, true_peak: bool = False,
                     limiter: bool = False, limiter_ms: float = 5.0):
        """Deliver every WHOLE utterance at ``target_lufs`` LUFS (ITU-R BS.1770-4 gated integrated loudness, mono,
        measured on the device on the floats the call delivers) under a ceiling of ``ceiling_db`` dB -- on the sample
        peak, or with ``true_peak`` on the true peak of BS.1770-4 Annex 2 as well (dBTP), measured on the device
        (include/piper_hip.h: pe_set_loudness, pe_set_loudness_ceiling). ``limiter``: where the ceiling and the target
        conflict, keep the target's gain and turn down only the neighbourhood of the peaks, with a zero-phase window of
        ``limiter_ms`` in [1, 10] (pe_set_loudness_limiter; either kind of ceiling). ``None``: off, the default -- every
        utterance scaled by ``32767 / max(0.01, peak)``; the kind of ceiling and the limiter are remembered. The floats
        never change; stream chunks keep their own rules. A refused call changes nothing."""
        kind = self.PEAK_TRUE if true_peak else self.PEAK_SAMPLE
        before = self.loudness_ceiling()[0]
        lim_before = self.loudness_limiter()
        loud_before = self.loudness()

        def attempt(rc):
            if not rc:
                return
            err = EngineError(self._lib.pe_last_error().decode(errors="replace"))
            # everything back as it was: the loudness off first, so that no intermediate combination is refused
            self._lib.pe_set_loudness(self._h, 0, 0.0, 0.0)
            self._lib.pe_set_loudness_limiter(self._h, 0, 0.0)
            self._lib.pe_set_loudness_ceiling(self._h, before)
            self._lib.pe_set_loudness_limiter(self._h, int(lim_before[0]), float(lim_before[1]))
            if loud_before[0] is not None:
                self._lib.pe_set_loudness(self._h, 1, float(loud_before[0]), float(loud_before[1]))
            raise err

        # (the limiter's window and the kind are checked before the loudness is touched; the true-peak kind goes in front
        # of the loudness, which it is refused with at a rate it does not cover)
        if limiter:
            attempt(self._lib.pe_set_loudness_limiter(self._h, 1, float(limiter_ms)))
        if target_lufs is None:
            attempt(self._lib.pe_set_loudness(self._h, 0, 0.0, 0.0))
            attempt(self._lib.pe_set_loudness_ceiling(self._h, kind))
        else:
            if true_peak:
                attempt(self._lib.pe_set_loudness_ceiling(self._h, kind))
            attempt(self._lib.pe_set_loudness(self._h, 1, float(target_lufs), float(ceiling_db)))
            if not true_peak:
                attempt(self._lib.pe_set_loudness_ceiling(self._h, kind))
        if not limiter:
            attempt(self._lib.pe_set_loudness_limiter(self._h, 0, 0.0))

    LOUD_SHAPED = 8

    def loudness_limiter(self):
        """(on, window_ms, W) of the look-ahead limiter (pe_get_loudness_limiter): W is the window in samples of the
        delivered rate (0 where the rate is unknown)."""
        on, ms, w = C.c_int32(), C.c_float(), C.c_int32()
        self._check(self._lib.pe_get_loudness_limiter(self._h, C.byref(on), C.byref(ms), C.byref(w)))
        return bool(on.value), float(ms.value), w.value

    def last_limiter(self):
        """(max_reduction, shaped_samples, trim) arrays of the last fetched whole-utterance call, one entry per utterance
        (pe_last_limiter); empty when that call ran without the limiter."""
        n = C.c_int32()
        self._check(self._lib.pe_last_limiter(self._h, None, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        r, c, t = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.pe_last_limiter(self._h, r.ctypes.data_as(fp), c.ctypes.data_as(C.POINTER(C.c_int32)),
                                              t.ctypes.data_as(fp), m, C.byref(n)))
        return r[:n.value], c[:n.value], t[:n.value]

    def debug_limiter(self, rows, fs: int, g, ceiling_db: float = -1.0, kind: int = 0, window_ms: float = 5.0, pad=0.0):
        """Test hook (pe_debug_limiter): the limiter kernel alone on ``rows``, a list of 1-D float arrays at rate ``fs``
        with one gain ``g[b]`` each; what lies behind a row's end in the staging matrix holds ``pad``. Returns (e, pcm):
        lists of one float32 / int16 array per row."""
        B = len(rows)
        valid = np.asarray([len(r) for r in rows], np.int32)
        stride = max(1, int(valid.max()))
        x = np.full((B, stride), pad, np.float32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.float32)
        gv = np.ascontiguousarray(g, np.float32)
        assert gv.shape == (B,)
        env, pcm = np.full((B, stride), np.nan, np.float32), np.zeros((B, stride), np.int16)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.pe_debug_limiter(self._h, x.ctypes.data_as(fp), B, stride, valid.ctypes.data_as(C.POINTER(C.c_int32)),
                                               int(fs), gv.ctypes.data_as(fp), float(ceiling_db), int(kind), float(window_ms),
                                               env.ctypes.data_as(fp), pcm.ctypes.data_as(C.POINTER(C.c_int16))))
        return [env[b, :valid[b]].copy() for b in range(B)], [pcm[b, :valid[b]].copy() for b in range(B)]

    def loudness_ceiling(self):
        """(kind, oversample, half_width) of the ceiling (pe_get_loudness_ceiling): ``PEAK_SAMPLE`` or ``PEAK_TRUE``, the
        interpolation factor of the true-peak measure at the delivered rate (0 where it has none) and its half-width."""
        k, q, w = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.pe_get_loudness_ceiling(self._h, C.byref(k), C.byref(q), C.byref(w)))
        return k.value, q.value, w.value

    def last_true_peak(self):
        """The true peak of every utterance of the last fetched whole-utterance call (pe_last_true_peak); empty when
        that call did not run with the true-peak ceiling."""
        n = C.c_int32()
        self._check(self._lib.pe_last_true_peak(self._h, None, 0, C.byref(n)))
        t = np.zeros(max(n.value, 1), np.float32)
        self._check(self._lib.pe_last_true_peak(self._h, t.ctypes.data_as(C.POINTER(C.c_float)), t.size, C.byref(n)))
        return t[:n.value]

    def debug_true_peak(self, rows, fs: int, pad=0.0):
        """Test hook (pe_debug_true_peak): the true-peak kernel alone on ``rows``, a list of 1-D float arrays at rate
        ``fs``; what lies behind a row's end in the staging matrix holds ``pad``. Returns one float per row."""
        B = len(rows)
        valid = np.asarray([len(r) for r in rows], np.int32)
        stride = max(1, int(valid.max()))
        x = np.full((B, stride), pad, np.float32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.float32)
        t = np.zeros(B, np.float32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.pe_debug_true_peak(self._h, x.ctypes.data_as(fp), B, stride,
                                                 valid.ctypes.data_as(C.POINTER(C.c_int32)), int(fs), t.ctypes.data_as(fp)))
        return t

    def loudness(self):
        """(target_lufs or None while off, ceiling_db) as set by ``set_loudness``."""
        on, t, c = C.c_int32(), C.c_float(), C.c_float()
        self._check(self._lib.pe_get_loudness(self._h, C.byref(on), C.byref(t), C.byref(c)))
        return (float(t.value) if on.value else None), float(c.value)

    def last_loudness(self):
        """(lufs, scale, peak, flags) arrays of the last fetched whole-utterance call, one entry per utterance
        (pe_last_loudness); empty when that call ran with the setting off. ``lufs`` is -inf where not measurable."""
        n = C.c_int32()
        self._check(self._lib.pe_last_loudness(self._h, None, None, None, None, 0, C.byref(n)))
        m = max(n.value, 1)
        L, s, p, f = np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.int32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.pe_last_loudness(self._h, L.ctypes.data_as(fp), s.ctypes.data_as(fp), p.ctypes.data_as(fp),
                                               f.ctypes.data_as(C.POINTER(C.c_int32)), m, C.byref(n)))
        return L[:n.value], s[:n.value], p[:n.value], f[:n.value]

    def debug_loudness(self, rows, fs: int, target_lufs: float = -23.0, ceiling_db: float = -1.0):
        """Test hook (pe_debug_loudness): the two loudness kernels alone on ``rows``, a list of 1-D float arrays at rate
        ``fs``. Returns (lufs, scale, flags) arrays, one entry per row."""
        B = len(rows)
        valid = np.asarray([len(r) for r in rows], np.int32)
        stride = max(1, int(valid.max()))
        x = np.zeros((B, stride), np.float32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.float32)
        L, s, f = np.zeros(B, np.float32), np.zeros(B, np.float32), np.zeros(B, np.int32)
        fp = C.POINTER(C.c_float)
        self._check(self._lib.pe_debug_loudness(
            self._h, x.ctypes.data_as(fp), B, stride, valid.ctypes.data_as(C.POINTER(C.c_int32)), int(fs),
            float(target_lufs), float(ceiling_db), L.ctypes.data_as(fp), s.ctypes.data_as(fp),
            f.ctypes.data_as(C.POINTER(C.c_int32))))
        return L, s, f

    def debug_stream_loudness(self, rows, fs: int, chunks, target_lufs: float = -23.0, ceiling_db: float = -1.0,
                              prior_lufs=None, ramp_samples: int = 0):
        """Test hook (pe_debug_stream_loudness): the stream loudness kernels and the chunk conversion, chunk after chunk,
        on ``rows``, a list of 1-D float arrays at rate ``fs``. ``chunks``: an int array [n_chunks][len(rows)] of chunk
        lengths (zeros allowed; a column's sum at most the row's length). Returns (lufs, g0, g1, flags), each
        [n_chunks][rows], and the int16 rows (a list; what no chunk covers is zero)."""
        B = len(rows)
        ch = np.ascontiguousarray(np.asarray(chunks, np.int32).reshape(-1, B))
        stride = max(1, max(len(r) for r in rows))
        x = np.zeros((B, stride), np.float32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.float32)
        K = ch.shape[0]
        L, g0, g1 = (np.zeros((K, B), np.float32) for _ in range(3))
        f = np.zeros((K, B), np.int32)
        pcm = np.zeros((B, stride), np.int16)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        prior = float("nan") if prior_lufs is None else float(prior_lufs)
        self._check(self._lib.pe_debug_stream_loudness(
            self._h, x.ctypes.data_as(fp), B, stride, int(fs), ch.ctypes.data_as(ip), K, float(target_lufs),
            float(ceiling_db), prior, int(ramp_samples), L.ctypes.data_as(fp), g0.ctypes.data_as(fp), g1.ctypes.data_as(fp),
            f.ctypes.data_as(ip), pcm.ctypes.data_as(C.POINTER(C.c_int16))))
        return L, g0, g1, f, [pcm[b, :len(r)].copy() for b, r in enumerate(rows)]

    def debug_stream_limiter(self, rows, fs: int, chunks, target_lufs: float = -23.0, ceiling_db: float = -1.0,
                             prior_lufs=None, ramp_samples: int = 0, window_ms: float = 5.0):
        """Test hook (pe_debug_stream_limiter): ``debug_stream_loudness`` with the stream limiter on; a row ends with its
        last chunk of length > 0. Returns (lufs, g0, g1, flags, delivered), each [n_chunks][rows], then per row e (float32
        per stream sample) and the int16 in delivery order (lists; what no call delivered is NaN / zero)."""
        B = len(rows)
        ch = np.ascontiguousarray(np.asarray(chunks, np.int32).reshape(-1, B))
        stride = max(1, max(len(r) for r in rows))
        x = np.zeros((B, stride), np.float32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.float32)
        K = ch.shape[0]
        L, g0, g1 = (np.zeros((K, B), np.float32) for _ in range(3))
        f, dl = np.zeros((K, B), np.int32), np.zeros((K, B), np.int32)
        env = np.full((B, stride), np.nan, np.float32)
        pcm = np.zeros((B, stride), np.int16)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        prior = float("nan") if prior_lufs is None else float(prior_lufs)
        self._check(self._lib.pe_debug_stream_limiter(
            self._h, x.ctypes.data_as(fp), B, stride, int(fs), ch.ctypes.data_as(ip), K, float(target_lufs),
            float(ceiling_db), prior, int(ramp_samples), float(window_ms), L.ctypes.data_as(fp), g0.ctypes.data_as(fp),
            g1.ctypes.data_as(fp), f.ctypes.data_as(ip), dl.ctypes.data_as(ip), env.ctypes.data_as(fp),
            pcm.ctypes.data_as(C.POINTER(C.c_int16))))
        return (L, g0, g1, f, dl, [env[b, :len(r)].copy() for b, r in enumerate(rows)],
                [pcm[b, :len(r)].copy() for b, r in enumerate(rows)])

    def _rates(self):
        nat, out, k = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.pe_get_output_rate(self._h, C.byref(nat), C.byref(out), C.byref(k)))
        return nat.value, out.value, k.value

    @property
    def output_rate(self) -> int:
        """The rate of what the engine delivers: the rate set by ``set_output_rate``, else the voice's own."""
        return self._rates()[1]

    @property
    def native_rate(self) -> int:
        return self._rates()[0]

    @property
    def resample_half_width(self) -> int:
        """K: native samples on each side of an output's position that its filter taps reach (0 at the native rate)."""
        return self._rates()[2]

    def debug_resample(self, rows, n0=None, count=None, origin=None) -> List[np.ndarray]:
        """Test hook (pe_debug_resample): the resampling kernel with the current rate pair on ``rows``, a list of 1-D float
        arrays of native samples. Row b's first sample has native index ``origin[b]`` (default 0); outputs ``n0[b]`` ..
        ``n0[b] + count[b] - 1`` are returned (default: all ceil(len * rate / native) outputs from 0)."""
        B = len(rows)
        nat, out, _ = self._rates()
        valid = np.asarray([len(r) for r in rows], np.int32)
        stride = max(1, int(valid.max()))
        x = np.zeros((B, stride), np.float32)
        for b, r in enumerate(rows):
            x[b, :len(r)] = np.asarray(r, np.float32)
        n0_a = np.zeros(B, np.int64) if n0 is None else np.ascontiguousarray(n0, np.int64)
        org_a = np.zeros(B, np.int64) if origin is None else np.ascontiguousarray(origin, np.int64)
        cnt_a = (np.asarray([-((-int(v) * out) // max(nat, 1)) for v in valid], np.int32) if count is None
                 else np.ascontiguousarray(count, np.int32))
        ostride = max(1, int(cnt_a.max()))
        y = np.zeros((B, ostride), np.float32)
        self._check(self._lib.pe_debug_resample(
            self._h, x.ctypes.data_as(C.POINTER(C.c_float)), B, stride, valid.ctypes.data_as(C.POINTER(C.c_int32)),
            n0_a.ctypes.data_as(C.POINTER(C.c_int64)), cnt_a.ctypes.data_as(C.POINTER(C.c_int32)),
            org_a.ctypes.data_as(C.POINTER(C.c_int64)), y.ctypes.data_as(C.POINTER(C.c_float)), ostride))
        return [y[b, :cnt_a[b]].copy() for b in range(B)]

    def debug_timing(self, logw_rows, scales=(0.667, 1.0, 0.8), timing: Optional[Timing] = None):
        """Test hook (pe_debug_timing): the timing-plan kernel alone on ``logw_rows``, a list of 1-D float arrays of logw,
        with ``scales`` (one triple or a (B, 3) array) and a ``Timing`` plan. Returns (durations, frames, w): per-utterance
        int32 arrays, an int32 array of B, per-utterance float32 arrays."""
        B = len(logw_rows)
        rows = [np.asarray(r, np.float32).reshape(-1) for r in logw_rows]
        offs = np.zeros(B + 1, np.int64)
        offs[1:] = np.cumsum([r.size for r in rows])
        lw = np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros(0, np.float32)
        per = _tiled_scales(scales, B)
        keep: list = []
        tref = None if timing is None else timing.pack(rows, keep)
        n = max(int(offs[-1]), 1)
        dur, frames, w = np.zeros(n, np.int32), np.zeros(max(B, 1), np.int32), np.zeros(n, np.float32)
        self._check(self._lib.pe_debug_timing(
            self._h, lw.ctypes.data_as(C.POINTER(C.c_float)), offs.ctypes.data_as(C.POINTER(C.c_int64)), B,
            per.ctypes.data_as(C.POINTER(C.c_float)), tref, dur.ctypes.data_as(C.POINTER(C.c_int32)),
            frames.ctypes.data_as(C.POINTER(C.c_int32)), w.ctypes.data_as(C.POINTER(C.c_float))))
        sl = [slice(int(offs[b]), int(offs[b + 1])) for b in range(B)]
        return [dur[s].copy() for s in sl], frames[:B].copy(), [w[s].copy() for s in sl]

    def set_seed(self, seed: int):
        self._lib.pe_set_seed(self._h, int(seed))

    def profile_enable(self, level=1):
        self._check(self._lib.pe_profile_enable(self._h, int(level)))

    def profile_reset(self):
        self._check(self._lib.pe_profile_reset(self._h))

    def profile(self):
        rows = []
        for i in range(self._lib.pe_profile_rows(self._h)):
            name, ms, fl, n = C.c_char_p(), C.c_double(), C.c_double(), C.c_int64()
            self._check(self._lib.pe_profile_get(self._h, i, C.byref(name), C.byref(ms), C.byref(fl), C.byref(n)))
            by = C.c_double()
            self._check(self._lib.pe_profile_bytes(self._h, i, C.byref(by)))
            rows.append({"name": name.value.decode(), "ms": ms.value, "flops": fl.value, "launches": n.value,
                         "bytes": by.value})
        return rows

    RNG_PITCH = 65536

    def debug_randn(self, site: int, call: int, n: int, row: int = 0) -> np.ndarray:
        """Test hook: n draws of the engine's own N(0,1) generator at sampling site 0/1, run counter `call`, from
        logical row `row` of the site's [row][65536] stream (row = utterance * channels + channel, column = id / frame)."""
        out = np.zeros(int(n), np.float32)
        self._check(self._lib.pe_debug_randn(self._h, int(site), int(call), int(row), int(n),
                                             out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    @property
    def run_launches(self) -> int:
        """Kernel launches (graph nodes) of the last run: the dependent launch chain of one step."""
        return int(self._lib.pe_run_launches(self._h))

    @property
    def speculation_stats(self):
        """(runs, misses) of the speculative stage-B sizing since the engine was created (include/piper_hip.h)."""
        runs, miss = C.c_int64(), C.c_int64()
        self._check(self._lib.pe_speculation_stats(self._h, C.byref(runs), C.byref(miss)))
        return int(runs.value), int(miss.value)

    def warmup(self, max_batch: int = 1, max_ids: int = 256, frames_per_id: float = 0.0, scales=None, sample_ids=None):
        """Pre-size the workspaces and (given a sample utterance) capture the single-utterance graphs of every id bucket
        up to max_ids -- include/piper_hip.h: pe_warmup."""
        sc = None if scales is None else (C.c_float * 3)(*[float(v) for v in scales])
        if sample_ids is None:
            self._check(self._lib.pe_warmup(self._h, int(max_batch), int(max_ids), float(frames_per_id), sc, None, 0))
            return
        ids = np.ascontiguousarray(sample_ids, np.int64)
        self._check(self._lib.pe_warmup(self._h, int(max_batch), int(max_ids), float(frames_per_id), sc,
                                        ids.ctypes.data_as(C.POINTER(C.c_int64)), ids.size))

    @property
    def graph_stats(self):
        """(graphs cached, captures since the engine was created) -- include/piper_hip.h: pe_graph_stats."""
        a, b = C.c_int64(), C.c_int64()
        self._check(self._lib.pe_graph_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    @property
    def xcc_pattern(self):
        """(XCC id of workgroups 0..63 of a probe launch at engine creation, round-robin period or 0) -- include/piper_hip.h."""
        xs = (C.c_int32 * 64)()
        per = C.c_int32()
        self._check(self._lib.pe_xcc_pattern(self._h, xs, C.byref(per)))
        return [int(v) for v in xs], int(per.value)

    @property
    def rng_calls(self) -> int:
        return int(self._lib.pe_rng_calls(self._h))

    @property
    def hip_stream(self) -> int:
        return int(self._lib.pe_stream(self._h) or 0)

    def debug_tensor(self, name: str, b: int = 0, capacity: int = 1 << 24) -> np.ndarray:
        out = np.zeros(capacity, np.float32)
        r, c = C.c_int32(), C.c_int32()
        self._check(self._lib.pe_debug_tensor(self._h, name.encode(), b, out.ctypes.data_as(C.POINTER(C.c_float)),
                                              capacity, C.byref(r), C.byref(c)))
        return out[: r.value * c.value].reshape(r.value, c.value).copy()


class StreamPool:
    """A live batch stream that listeners join and leave (pe_stream_pool_*). The latents of the utterances in flight are
    resident in storage the pool owns, so every other call on the engine may run between two chunks. ``halo``: the
    generator's receptive half-width in frames. ``frames`` / ``frames_done``: per slot, the utterance's frame count and the
    frames delivered so far (a finished slot's stay readable until the slot is reused). ``free_slots``: the slots a join
    may take, in the order it takes them. The int16 level follows the engine's ``set_stream_gain``: in the running mode
    every slot carries its own level, reset by the join that takes the slot."""

    def __init__(self, engine: Engine, slots: int, max_frames: int):
        self._eng, self.slots, self.max_frames, self._open = engine, int(slots), int(max_frames), False
        halo = C.c_int32()
        engine._check(engine._lib.pe_stream_pool_open(engine._h, self.slots, self.max_frames, C.byref(halo)))
        self.halo, self._open = halo.value, True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self._open and self._eng._h:
            self._open = False
            self._eng._check(self._eng._lib.pe_stream_pool_close(self._eng._h))
        self._open = False

    def _state(self):
        n = C.c_int32()
        arr = np.zeros((3, max(self.slots, 1)), np.int32)
        p = [arr[i].ctypes.data_as(C.POINTER(C.c_int32)) for i in range(3)]
        self._eng._check(self._eng._lib.pe_stream_pool_state(self._eng._h, C.byref(n), p[0], p[1], p[2]))
        if n.value != self.slots:
            raise EngineError("no stream pool open on this handle")
        return arr[:, :self.slots]

    @property
    def frames(self) -> np.ndarray:
        return self._state()[0].copy()

    @property
    def frames_done(self) -> np.ndarray:
        return self._state()[1].copy()

    @property
    def free_slots(self) -> list:
        return [int(s) for s in np.flatnonzero(self._state()[2] == 0)]

    def join(self, id_lists, scales=(0.667, 1.0, 0.8), sids=None, noise_w=None, noise_z=None,
             timing: Optional[Timing] = None, seeds=None, speakers=None) -> list:
        """Begin the utterances of ``id_lists`` and give each a free slot, lowest first, in input order; returns the slots.
        ``scales``: one triple, or a (B, 3) array of per-utterance triples. Fails as a whole, the pool unchanged, when
        there are too few free slots or an utterance has more than ``max_frames`` frames. ``timing``: a ``Timing`` plan
        (pe_stream_pool_join_timed). ``seeds``: one int or None per newcomer (pe_stream_pool_join_seeded). ``speakers``:
        one entry per newcomer as in ``Engine.synthesize_batch`` (pe_stream_pool_join_blended)."""
        eng, n = self._eng, len(id_lists)
        keep0: list = []
        sids, blend = pack_speakers(speakers, sids, n, eng.speaker_dim, keep0)
        ids, offs = eng._pack(id_lists)
        per = per_utterance_scales(scales, n)
        if per is None:
            per = np.ascontiguousarray(np.tile(np.asarray(scales, np.float32), (max(n, 1), 1)))
        keep: list = [per]
        nref = eng._noise(noise_w, noise_z, keep)
        sid_arr = None
        if sids is not None:
            sid_np = np.ascontiguousarray(sids, np.int64)
            keep.append(sid_np)
            sid_arr = sid_np.ctypes.data_as(C.POINTER(C.c_int64))
        slot_of, frames = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        entry, extra = eng._lib.pe_stream_pool_join, ()
        if timing is not None:
            entry, extra = eng._lib.pe_stream_pool_join_timed, (timing.pack(id_lists, keep),)
        if seeds is not None:
            entry, extra = eng._lib.pe_stream_pool_join_seeded, (extra[0] if extra else None, pack_seeds(seeds, n, keep))
        if blend is not None:
            keep += keep0
            entry, extra = eng._lib.pe_stream_pool_join_blended, ((extra + (None, None))[0], (extra + (None, None))[1], blend)
        eng._check(entry(
            eng._h, ids.ctypes.data_as(C.POINTER(C.c_int64)), offs.ctypes.data_as(C.POINTER(C.c_int64)), n,
            per.ctypes.data_as(C.POINTER(C.c_float)), sid_arr, nref, slot_of.ctypes.data_as(C.POINTER(C.c_int32)),
            frames.ctypes.data_as(C.POINTER(C.c_int32)), *extra))
        return [int(s) for s in slot_of[:n]]

    def next(self, chunk_frames: int = 45, per_slot=None, want_audio: bool = True) -> dict:
        """The next chunk of every listener, one batched vocoder pass: ``{slot: (float chunk or None, int16 chunk)}`` for the
        slots that got samples (a ``Chunk``: the pair, with ``.codes`` under a G.711 sample format) -- empty when no slot has frames left (with the stream limiter also when every listener only
        held samples back: ask ``frames_done`` / ``free_slots``). ``per_slot``: ``{slot: frames}`` (or an array of
        ``slots`` entries, 0 = default) overriding ``chunk_frames``, e.g. a short first chunk for a newcomer."""
        eng, S = self._eng, self.slots
        ps = None
        if per_slot is not None:
            ps_np = np.zeros(S, np.int32)
            if isinstance(per_slot, dict):
                for s, c in per_slot.items():
                    ps_np[int(s)] = int(c)
            else:
                ps_np[:] = np.asarray(per_slot, np.int32)
            ps = ps_np.ctypes.data_as(C.POINTER(C.c_int32))
        ch = L.PeStreamChunk()
        eng._check(eng._lib.pe_stream_pool_next(eng._h, int(chunk_frames), ps, int(bool(want_audio)), C.byref(ch)))
        offs = np.frombuffer(C.string_at(ch.sample_offsets, 8 * (S + 1)), np.int64)
        total = int(offs[-1])
        if total == 0:
            return {}
        p = np.frombuffer(bytearray(C.string_at(ch.pcm, 2 * total)), np.int16)
        a = np.frombuffer(bytearray(C.string_at(ch.audio, 4 * total)), np.float32) if ch.audio else None
        c = eng._last_codes(1)
        return {s: Chunk(None if a is None else a[offs[s]:offs[s + 1]], p[offs[s]:offs[s + 1]], None if c is None else c[s])
                for s in range(S) if offs[s + 1] > offs[s]}

    def leave(self, slot: int):
        """Free an occupied slot at once (the listener hung up)."""
        self._eng._check(self._eng._lib.pe_stream_pool_leave(self._eng._h, int(slot)))


def loudness_filter(fs: int, lib=None) -> np.ndarray:
    """The K-weighting biquads of ITU-R BS.1770-4 at rate ``fs`` (pe_loudness_filter; host only): float64
    [shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2]."""
    lib = lib if lib is not None else L.get_lib()
    out = np.zeros(10, np.float64)
    if lib.pe_loudness_filter(int(fs), out.ctypes.data_as(C.POINTER(C.c_double))):
        raise EngineError(lib.pe_last_error().decode(errors="replace"))
    return out


def true_peak_filter(fs: int, lib=None):
    """The interpolator of the true-peak measure at rate ``fs`` (pe_true_peak_filter; host only): (Q, K, float64 table
    [Q][2 K]), row ph holding the taps of the outputs ``c Q + ph`` on ``x[c - K + 1 .. c + K]``."""
    lib = lib if lib is not None else L.get_lib()
    q, k, n = C.c_int32(), C.c_int32(), C.c_int64()
    if lib.pe_true_peak_filter(int(fs), C.byref(q), C.byref(k), None, 0, C.byref(n)):
        raise EngineError(lib.pe_last_error().decode(errors="replace"))
    out = np.zeros(n.value, np.float64)
    if lib.pe_true_peak_filter(int(fs), C.byref(q), C.byref(k), out.ctypes.data_as(C.POINTER(C.c_double)), out.size, C.byref(n)):
        raise EngineError(lib.pe_last_error().decode(errors="replace"))
    return q.value, k.value, out.reshape(q.value, 2 * k.value)


def limiter_window(fs: int, window_ms: float, lib=None):
    """The look-ahead limiter's window at rate ``fs`` (pe_limiter_window; host only): (W, float64 weights [2 W + 1])."""
    lib = lib if lib is not None else L.get_lib()
    w, n = C.c_int32(), C.c_int64()
    if lib.pe_limiter_window(int(fs), float(window_ms), C.byref(w), None, 0, C.byref(n)):
        raise EngineError(lib.pe_last_error().decode(errors="replace"))
    out = np.zeros(n.value, np.float64)
    if lib.pe_limiter_window(int(fs), float(window_ms), C.byref(w), out.ctypes.data_as(C.POINTER(C.c_double)), out.size, C.byref(n)):
        raise EngineError(lib.pe_last_error().decode(errors="replace"))
    return w.value, out


def _g711(entry, fmt: str, x: np.ndarray, out_dtype, in_ctype, out_ctype, lib=None) -> np.ndarray:
    lib = lib if lib is not None else L.get_lib()
    if fmt not in ("ulaw", "alaw"):
        raise EngineError(f"G.711 format {fmt!r}: 'ulaw' or 'alaw'")
    out = np.zeros(x.size, out_dtype)
    if getattr(lib, entry)(1 if fmt == "ulaw" else 2, x.ctypes.data_as(C.POINTER(in_ctype)),
                           out.ctypes.data_as(C.POINTER(out_ctype)), x.size):
        raise EngineError(lib.pe_last_error().decode(errors="replace"))
    return out


def g711_encode(fmt: str, pcm, lib=None) -> np.ndarray:
    """int16 samples -> G.711 codes (pe_g711_encode; host only): the law of the ITU-T G.191 tools, ``fmt`` "ulaw" / "alaw"."""
    return _g711("pe_g711_encode", fmt, np.ascontiguousarray(pcm, np.int16).ravel(), np.uint8, C.c_int16, C.c_uint8, lib)


def g711_decode(fmt: str, codes, lib=None) -> np.ndarray:
    """G.711 codes -> int16 samples (pe_g711_decode; host only), the expanders of the same tools."""
    return _g711("pe_g711_decode", fmt, np.ascontiguousarray(codes, np.uint8).ravel(), np.int16, C.c_uint8, C.c_int16, lib)
