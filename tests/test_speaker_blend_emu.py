"""Speaker blends and caller-supplied speaker vectors (include/piper_hip.h: pe_blend) on the CPU, through the
kernel emulator's build of the engine: the truth against the oracle, the two bit-for-bit consequences on both input paths, the
vector law, independence of the batch, streams and the pool, coalescer and group, the refusals, the launch count and the host
layers (PiperVoice, piper_amd.infer, SynthesisConfig through tests/cpp/test_speaker_blend.cpp). tests/speaker_blend_case.py
holds what this file shares with tests/test_gpu_speaker_blend.py.

The emulator runs the vocoder slowly, so everything but the truth test uses a few ids per utterance."""
import io
import json
import os
import re
import subprocess

import ctypes as C
import numpy as np
import pytest

import one_utterance_truth_case as U
import seeds_case as S
import speaker_blend_case as K
from piper_amd import _lib as L, weights as W
from piper_amd.engine import Engine, EngineError

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
VOICE = "tiny-ms"          # gin 16, 4 speakers, weights seed 1234


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()


@pytest.fixture(scope="module")
def eng(emu_lib):
    return U.engine_for(VOICE, {}, lib=emu_lib)


def _short(cfg, lens=(4, 3, 5)):
    return K.ids_of(cfg, lens)


# ---- 1. truth
def test_truth_against_the_oracle(eng):
    """Three blends -- inside the table's hull, a single component, an extrapolation -- with injected noise: durations equal
    the oracle's on the one-row table of each utterance's g, audio within the emulator tests' gate for plain speakers, and
    the durations of utterances 0 and 2 are not their first component's."""
    cfg, w = U.voice(VOICE)
    ids = K.ids_of(cfg)
    nw, nz = K.noise(cfg, 3, max(K.LENS))
    t = K.truth(w, cfg, (VOICE, 1234), ids, K.SCALES, nw, nz, K.SPEAKERS)
    K.check_margin(t, "emu truth")
    r = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz, speakers=K.SPEAKERS)
    d = np.split(eng.durations(), np.cumsum(K.LENS)[:-1])
    assert list(t[0]["durations"][:3]) == [4, 8, 3] and list(t[0]["first"][:3]) == [5, 12, 3]
    for b in range(3):
        assert np.array_equal(t[b]["durations"], t[b]["d_only"])
        assert np.array_equal(d[b], t[b]["durations"]), (b, d[b], t[b]["durations"])
        assert r.audio[b].shape == t[b]["audio"].shape
        err = float(np.max(np.abs(r.audio[b] - t[b]["audio"])))
        print(f"[emu truth] utterance {b}: max |audio - oracle| {err:.3e}")
        assert err < 1e-4, (b, err)
    for b in (0, 2):
        assert not np.array_equal(t[b]["durations"], t[b]["first"]), b


# ---- 2. bit for bit
@pytest.mark.parametrize("path", ["copied", "zero-copy"])
def test_unit_blend_and_table_row_are_the_plain_call(emu_lib, path):
    """{s: 1.0} and the vector speaker_embedding(s) against sids=[s]: audio, PCM and durations np.array_equal. Once with injected
    noise on an engine whose input block is copied to the device (PIPER_HIP_IDS_ZC=0: the path of calls beyond 65 536 padded
    ids), once with seeds and no injected noise on the zero-copy path. B = 1, and B = 3 with the three kinds mixed."""
    cfg, _ = U.voice(VOICE)
    eng = U.engine_for(VOICE, {"PIPER_HIP_IDS_ZC": 0} if path == "copied" else {}, lib=emu_lib)
    ids = _short(cfg)
    nw, nz = K.noise(cfg, 3, 5, seed=4)

    def call(n, **kw):
        extra = dict(noise_w=nw[:n], noise_z=nz[:n]) if path == "copied" else dict(seeds=[11, 12, 13][:n])
        r = eng.synthesize_batch(ids[:n], K.SCALES, **extra, **kw)
        return r, eng.durations()

    def same(a, b, what):
        (ra, da), (rb, db) = a, b
        assert np.array_equal(da, db), what
        for u in range(len(ra.audio)):
            assert np.array_equal(ra.audio[u], rb.audio[u]) and np.array_equal(ra.pcm[u], rb.pcm[u]), (what, u)

    s = 2
    plain = call(1, sids=[s])
    same(call(1, speakers=[{s: 1.0}]), plain, "unit blend")
    same(call(1, speakers=[eng.speaker_embedding(s)]), plain, "table row as a vector")
    plain3 = call(3, sids=[3, 1, 0])
    same(call(3, speakers=[{3: 1.0}, eng.speaker_embedding(1), 0]), plain3, "three kinds in one call")
    other = call(1, speakers=[{s: 0.5, 0: 0.5}])
    assert not np.array_equal(other[0].audio[0], plain[0].audio[0]) or other[0].audio[0].shape != plain[0].audio[0].shape


# ---- 3. the vector law
def test_vector_law_in_a_call_and_alone(eng, emu_lib):
    """debug_tensor("g") of a mixed call against the law in f64 (bound in speaker_blend_case), exact for the vector and the
    plain id; then pe_debug_blend alone at gin 512 with 12 speakers: 64 utterances, counts cycling -1, 0, 1, 8."""
    cfg, w = U.voice(VOICE)
    E = K.table(w)
    assert eng.speaker_dim == cfg.gin == 16
    for s in range(cfg.n_speakers):
        assert np.array_equal(eng.speaker_embedding(s), E[s])
    ids = _short(cfg, (2, 2, 2, 2))
    v = np.random.default_rng(8).standard_normal(16).astype(np.float32)
    speakers = [[(0, 1.5), (1, -0.5), (0, 0.25)], v, 3, {2: -2.0}]
    eng.synthesize_batch(ids, (0.0, 1.0, 0.0), speakers=speakers)
    for b, sp in enumerate(speakers):
        g = eng.debug_tensor("g", b)
        assert g.shape == (1, 16)
        K.check_vector(g, E, sp, f"emu g utt {b}")
    eng.synthesize_batch(ids[:2], (0.0, 1.0, 0.0), sids=[1, 2])
    assert np.array_equal(eng.debug_tensor("g", 1)[0], E[2])
    out = eng.debug_blend(speakers)
    for b, sp in enumerate(speakers):
        K.check_vector(out[b], E, sp, f"emu debug_blend utt {b}")

    cfg5 = W.preset(VOICE, gin=512, n_speakers=12)
    w5 = W.synthetic_weights(cfg5, 1234)
    big = Engine(blob=W.pack_blob(cfg5, w5), lib=emu_lib)
    try:
        E5 = K.table(w5)
        assert big.speaker_dim == 512 and E5.shape == (12, 512)
        sp5 = K.debug_cases(E5)
        out = big.debug_blend(sp5)
        assert out.shape == (64, 512)
        worst = max(K.check_vector(out[b], E5, sp, f"emu gin 512 utt {b}") for b, sp in enumerate(sp5))
        print(f"[emu debug_blend 64 x 8 x 512] worst |g - g64| / bound {worst:.3f}")
    finally:
        big.close()


# ---- 4. independence
def test_independent_of_the_batch(eng):
    """A seeded blended utterance alone, as row 0 and as row 2 of a call of three with plain and vector neighbours: g bit for
    bit, durations and frames equal, PCM within the seeded-independence tests' bound."""
    cfg, w = U.voice(VOICE)
    ids = _short(cfg)
    sp = {1: 0.7, 3: 0.3}
    v = K.table(w)[0] * np.float32(0.5)
    alone = eng.synthesize_batch(ids[:1], K.SCALES, seeds=[5], speakers=[sp])
    d0, g0 = eng.durations(), eng.debug_tensor("g", 0)
    first = eng.synthesize_batch([ids[0], ids[1], ids[2]], K.SCALES, seeds=[5, None, 7], speakers=[sp, 2, v])
    d1, g1 = eng.durations()[:4], eng.debug_tensor("g", 0)
    last = eng.synthesize_batch([ids[1], ids[2], ids[0]], K.SCALES, seeds=[None, 7, 5], speakers=[None, v, sp])
    d2, g2 = eng.durations()[-4:], eng.debug_tensor("g", 2)
    assert np.array_equal(g0, g1) and np.array_equal(g0, g2)
    assert np.array_equal(d0, d1) and np.array_equal(d0, d2)
    assert alone.frames[0] == first.frames[0] == last.frames[2]
    S.pcm_close(first.pcm[0], alone.pcm[0], "emu blend as row 0")
    S.pcm_close(last.pcm[2], alone.pcm[0], "emu blend as row 2")


# ---- 5. streams
def test_streams_and_pool(eng):
    """stream, stream_batch and a pool join with a blend: the chunks concatenate to the blended whole-utterance call within
    1e-5; a slot used by a blended utterance, left, and taken by a plain one delivers the plain utterance's own audio."""
    cfg, _ = U.voice(VOICE)
    ids = _short(cfg, (3, 2))
    sp = {0: 1.5, 1: -0.5}
    zero = (0.0, 1.0, 0.0)
    whole = eng.synthesize_batch(ids, zero, speakers=[sp, 2])
    plain = eng.synthesize_batch(ids[:1], zero, sids=[3])
    assert whole.audio[0].shape != plain.audio[0].shape or not np.array_equal(whole.audio[0], plain.audio[0])

    def close(a, ref, what):
        assert a.shape == ref.shape, (what, a.shape, ref.shape)
        err = float(np.max(np.abs(a - ref))) if a.size else 0.0
        print(f"[emu {what}] max |chunks - whole| {err:.3e}")
        assert err < 1e-5, (what, err)

    close(np.concatenate([c[0] for c in eng.stream(ids[0], zero, chunk_frames=12, speaker=sp)]), whole.audio[0], "stream")
    got = [[], []]
    for item in eng.stream_batch(ids, zero, chunk_frames=12, speakers=[sp, 2]):
        for b in range(2):
            got[b].append(item[b][0])
    for b in range(2):
        close(np.concatenate(got[b]), whole.audio[b], f"stream_batch utt {b}")

    def drain(pool, slot):
        out = []
        while True:
            step = pool.next(12)
            if not step:
                return np.concatenate(out)
            if slot in step:
                out.append(step[slot][0])
    with eng.stream_pool(2, 256) as pool:
        slot = pool.join(ids[:1], zero, speakers=[sp])[0]
        close(drain(pool, slot), whole.audio[0], "pool join")
        slot2 = pool.join(ids[:1], zero, speakers=[sp])[0]
        pool.next(6)
        pool.leave(slot2)
        slot3 = pool.join(ids[:1], zero, sids=[3])[0]
        assert slot3 == slot2
        close(drain(pool, slot3), plain.audio[0], "pool slot after a blended tenant")


# ---- 6. coalescer and group
def test_coalescer_and_group(emu_lib, monkeypatch):
    """A blended request merged with two plain ones (the leader waits for a full batch of three) equals its own B = 1 blended
    call under the coalescer tests' gate; a group of two members carries each utterance's blend to the member that runs it."""
    import threading
    from piper_amd.group import Coalescer, EngineGroup
    cfg, w = U.voice(VOICE)
    ids = _short(cfg)
    sp = {1: 0.7, 3: 0.3}
    zero = (0.0, 1.0, 0.0)
    eng = U.engine_for(VOICE, {}, lib=emu_lib, fresh=True)
    co = Coalescer(eng, max_batch=3, max_wait_us=60000000, mix_scales=True)
    out, errs = [None] * 3, []

    def work(i):
        try:
            out[i] = co.synthesize(ids[i], zero, sid=None if i == 0 else i, speaker=sp if i == 0 else None)
        except Exception as ex:              # noqa: BLE001
            errs.append(ex)
    try:
        th = [threading.Thread(target=work, args=(i,)) for i in range(3)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert not errs, errs
        assert co.stats == (1, 3)
        one = eng.synthesize(ids[0], zero, speaker=sp)
        pcm, frames, _, bs = out[0]
        assert bs == 3 and frames == int(one.frames[0])
        S.pcm_close(pcm, one.pcm[0], "emu coalesced blend")
        for i in (1, 2):
            p1 = eng.synthesize(ids[i], zero, sid=i)
            assert out[i][1] == int(p1.frames[0])
            S.pcm_close(out[i][0], p1.pcm[0], f"emu coalesced plain {i}")
        with pytest.raises(EngineError, match="utterance 0.*component 1"):
            co.synthesize(ids[0], zero, speaker=[(0, 1.0), (9, 1.0)])
    finally:
        co.close()
    monkeypatch.setenv("PIPER_HIP_GROUP_COALESCE", "0")
    grp = EngineGroup(W.pack_blob(cfg, w), [0, 0], lib=emu_lib)
    try:
        v = K.table(w)[2] * np.float32(1.25)
        speakers = [sp, v]
        r = grp.synthesize_batch(ids[:2], zero, speakers=speakers)
        assign = grp.assignment(2)
        assert sorted(assign) == [0, 1]
        one = eng.synthesize_batch(ids[:2], zero, speakers=speakers)
        for u in range(2):
            K.check_vector(grp.engine(assign[u]).debug_tensor("g", 0), K.table(w), speakers[u], f"emu group utt {u}")
            assert r.frames[u] == one.frames[u]
            S.pcm_close(r.pcm[u], one.pcm[u], f"emu group utt {u}")
    finally:
        grp.close()
        eng.close()


# ---- 7. refusals
def _raw_blend(count, sid=None, weight=None, vector=None):
    keep = [np.ascontiguousarray(count, np.int32)]
    b = L.PeBlend()
    b.count = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    if sid is not None:
        keep.append(np.ascontiguousarray(sid, np.int64))
        b.sid = keep[-1].ctypes.data_as(C.POINTER(C.c_int64))
    if weight is not None:
        keep.append(np.ascontiguousarray(weight, np.float32))
        b.weight = keep[-1].ctypes.data_as(C.POINTER(C.c_float))
    if vector is not None:
        keep.append(np.ascontiguousarray(vector, np.float32))
        b.vector = keep[-1].ctypes.data_as(C.POINTER(C.c_float))
    return b, keep


def test_refusals(eng, emu_lib):
    """Every refused case raises with the utterance (and the component) in the message, before anything of the engine
    changes: a stream begun before the refused calls delivers its remaining chunks, and the next call is served."""
    cfg, _ = U.voice(VOICE)
    ids = _short(cfg, (3, 2))
    zero = (0.0, 1.0, 0.0)
    whole = eng.synthesize_batch(ids[:1], zero, sids=[1])
    chunks = eng.stream(ids[0], zero, sid=1, chunk_frames=8)
    got = [next(chunks)[0]]
    nan_v = np.zeros((2, 16), np.float32)
    nan_v[1, 7] = np.inf
    cases = [
        ([0, 9], None, None, None, r"utterance 1.*count 9"),
        ([-2, 0], None, None, None, r"utterance 0.*count -2"),
        ([1, 2], [0, 1, 4], [1.0, 1.0, 1.0], None, r"utterance 1, blend component 1.*speaker id 4"),
        ([2, 0], [0, -1], [1.0, 1.0], None, r"utterance 0, blend component 1.*speaker id -1"),
        ([1, 2], [0, 1, 2], [1.0, 1.0, np.nan], None, r"utterance 1, blend component 1.*not finite"),
        ([0, -1], None, None, nan_v, r"utterance 1.*element 7.*not finite"),
        ([0, -1], None, None, None, r"utterance 1.*vector is null"),
        ([0, 2], None, [1.0, 1.0], None, r"utterance 1.*sid is null"),
        ([2, 0], [0, 1], None, None, r"utterance 0.*weight is null"),
    ]
    flat, offs = eng._pack(ids)
    sc = np.ascontiguousarray(np.tile(np.asarray(zero, np.float32), (2, 1)))
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    args = (eng._h, flat.ctypes.data_as(i64p), offs.ctypes.data_as(i64p), 2, sc.ctypes.data_as(f32p), None, None)
    for count, sid, weight, vector, msg in cases:
        b, keep = _raw_blend(count, sid, weight, vector)
        res = L.PeResult()
        assert emu_lib.pe_synthesize_batch_blended(*args, C.byref(res), None, None, C.byref(b)) != 0, msg
        err = emu_lib.pe_last_error().decode()
        assert re.search(msg, err), (msg, err)
        assert emu_lib.pe_upload_blended(*args, None, None, C.byref(b)) != 0 and re.search(msg, emu_lib.pe_last_error().decode())
    with pytest.raises(EngineError, match="utterance 0, blend component 0"):
        eng.synthesize_batch(ids[:1], zero, speakers=[{7: 1.0}])
    with pytest.raises(EngineError, match="utterance 0"):
        eng.debug_blend([{7: 1.0}])
    with pytest.raises(ValueError, match="utterance 0"):
        eng.synthesize_batch(ids[:1], zero, sids=[1], speakers=[{1: 1.0}])
    with pytest.raises(ValueError):
        eng.synthesize_batch(ids[:1], zero, speakers=[np.zeros(15, np.float32)])
    # the stream begun before all of this goes on
    got += [c[0] for c in chunks]
    a = np.concatenate(got)
    assert a.shape == whole.audio[0].shape and float(np.max(np.abs(a - whole.audio[0]))) < 1e-5
    again = eng.synthesize_batch(ids[:1], zero, sids=[1])
    assert np.array_equal(again.audio[0], whole.audio[0])
    # a single-speaker voice refuses every blend
    single = U.engine_for("tiny", {}, lib=emu_lib)
    assert single.speaker_dim == 0
    with pytest.raises(EngineError, match="single-speaker"):
        single.synthesize_batch([ids[1]], zero, speakers=[{0: 1.0}])
    with pytest.raises(EngineError):
        single.speaker_embedding(0)


# ---- 8. launches
def test_one_launch_more(eng):
    """Level-2 profile: a plain multi-speaker call has no speaker_blend_kernel row, a blended one exactly one launch of it,
    and the blended B = 1 call takes at most the plain one's launches + 1."""
    cfg, _ = U.voice(VOICE)
    ids = _short(cfg, (3,))
    zero = (0.0, 1.0, 0.0)
    plain = S.profiled_names(eng, lambda: eng.synthesize_batch(ids, zero, sids=[1]))
    n_plain = eng.run_launches
    blended = S.profiled_names(eng, lambda: eng.synthesize_batch(ids, zero, speakers=[{1: 0.5, 2: 0.5}]))
    n_blend = eng.run_launches
    assert "speaker_blend_kernel" not in plain and plain["cond_kernel"] == blended["cond_kernel"]
    assert blended["speaker_blend_kernel"] == 1
    assert {k: v for k, v in blended.items() if k != "speaker_blend_kernel"} == plain
    assert n_blend <= n_plain + 1, (n_blend, n_plain)
    # pe_run repeated on a blended upload keeps the blend; the next upload drops it
    eng.upload(ids, zero, speakers=[{1: 0.5, 2: 0.5}])
    eng.run()
    a = eng.fetch().audio[0].copy()
    eng.run()
    assert np.array_equal(eng.fetch().audio[0], a)
    eng.upload(ids, zero, sids=[1])
    eng.run()
    b = eng.fetch().audio[0]
    assert a.shape != b.shape or not np.array_equal(a, b)
    assert np.array_equal(eng.debug_tensor("g", 0)[0], eng.speaker_embedding(1))


# ---- 9. higher layers
def test_voice_and_driver(emu_lib, tmp_path, monkeypatch):
    """PiperVoice keywords (names through speaker_id_map, the both-given error); piper_amd.infer's --speaker-blend and
    per-line keys: what reaches Engine.synthesize_batch, and the error that names the line."""
    from piper_amd import infer
    from piper_amd.config import PiperConfig
    from piper_amd.voice import PiperVoice
    model = os.path.join(U.ROOT, "tests", "golden", "tinyhms_voice.onnx")
    conf = PiperConfig.from_dict(json.load(open(model + ".json", encoding="utf-8")))
    voice = PiperVoice(session=Engine(onnx_path=model, lib=emu_lib), config=conf)
    ids = [int(x) for x in W.synthetic_phoneme_ids(2, 3, id_max=39)]
    eng = voice.session
    eng.set_seed(1)
    zero = dict(noise_scale=0.0, noise_w=0.0, length_scale=0.4)      # (short: the emulator runs the vocoder slowly)
    a = voice.synthesize_ids_to_raw(ids, speaker_blend={"spk1": 0.7, 3: 0.3}, **zero)
    assert a == eng.synthesize(ids, (0.0, 0.4, 0.0), speaker=[(1, 0.7), (3, 0.3)]).pcm[0].tobytes()
    v = eng.speaker_embedding(2)
    plain = voice.synthesize_ids_to_raw(ids, speaker_id=2, **zero)
    assert voice.synthesize_ids_to_raw(ids, speaker_vector=v, **zero) == plain != a
    two = voice.synthesize_ids_batch_to_raw([ids, ids], speaker_blend=[{"spk1": 0.7, "spk3": 0.3}, None],
                                            speaker_vector=[None, v], **zero)
    assert two[0] == a and two[1] == plain
    for kw in (dict(speaker_id=1, speaker_blend={1: 1.0}), dict(speaker_id=1, speaker_vector=v),
               dict(speaker_blend={1: 1.0}, speaker_vector=v)):
        with pytest.raises(ValueError):
            voice.synthesize_ids_to_raw(ids, **kw)
    with pytest.raises(ValueError):
        voice.synthesize_ids_to_raw(ids, speaker_blend={"nobody": 1.0})
    voice.session.close()

    seen = []
    real = Engine.synthesize_batch

    def spy(self, id_lists, scales=(0.667, 1.0, 0.8), **kw):
        seen.append((kw.get("sids"), kw.get("speakers")))
        return real(self, id_lists, scales, **kw)
    monkeypatch.setattr(Engine, "synthesize_batch", spy)
    vec = [float(x) for x in v]
    lines = [json.dumps({"phoneme_ids": ids}), "", json.dumps({"phoneme_ids": ids, "speaker_blend": {"2": 1.0}}),
             json.dumps({"phoneme_ids": ids, "speaker_vector": vec}), json.dumps({"phoneme_ids": ids, "speaker_id": 2})]
    out = tmp_path / "wavs"
    assert infer.main(["--model", model, "--output-dir", str(out), "--sample-rate", "16000", "--batch", "4", "--noise-scale", "0",
                       "--noise-scale-w", "0", "--length-scale", "0.4", "--speaker-blend", "spk1:0.7,3:0.3"], stdin=io.StringIO("\n".join(lines)), lib=emu_lib) == 0
    assert len(seen) == 1
    sids, speakers = seen[0]
    assert sids is None and speakers[0] == [(1, 0.7), (3, 0.3)] and speakers[1] == [(2, 1.0)] and speakers[3] == 2
    assert np.array_equal(np.asarray(speakers[2], np.float32), v)
    import wave
    wavs = []
    for k in (0, 2, 3, 4):
        with wave.open(str(out / f"{k}.wav"), "rb") as wv:
            wavs.append(wv.readframes(wv.getnframes()))
    assert wavs[0] == a and wavs[1] == wavs[2] == wavs[3] == plain
    bad = [lines[0], json.dumps({"phoneme_ids": ids, "speaker_id": 1, "speaker_blend": {"2": 1.0}})]
    with pytest.raises(ValueError, match="line 2"):
        infer.main(["--model", model, "--output-dir", str(out)], stdin=io.StringIO("\n".join(bad)), lib=emu_lib)
    seen.clear()
    assert infer.main(["--model", model, "--output-dir", str(tmp_path / "plain")], stdin=io.StringIO(lines[0]), lib=emu_lib) == 0
    assert seen[0][1] is None


def test_synthesis_config_through_piper_hpp():
    """tests/cpp/test_speaker_blend.cpp against the emulator build: SynthesisConfig::speakerBlend and ::speakerVector in
    synthesize, synthesizeBatch and textToAudio, and the three refused combinations."""
    exe = os.path.join(U.ROOT, "tests", "cpp", "test_speaker_blend_emu")
    deps = [EMU, os.path.join(U.ROOT, "tests", "cpp", "test_speaker_blend.cpp"), os.path.join(U.ROOT, "include", "piper.hpp"),
            os.path.join(U.ROOT, "include", "piper_hip.h")]
    if not all(os.path.exists(f) for f in [exe] + deps) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["make", "-C", U.ROOT, "emu", "tests/cpp/test_speaker_blend_emu"], stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, os.path.join(U.ROOT, "tests", "golden", "tinyhms_voice.onnx")], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    assert re.search(r"^OK unit=1 row=1 blend_differs=1 batch=1 text=1 refused=3", out.stdout, re.M), out.stdout
