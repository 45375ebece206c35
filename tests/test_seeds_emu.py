"""Per-utterance noise seeds (include/piper_hip.h: pe_seeds) on the CPU, through the kernel emulator's build of the engine:
the law in every kernel that draws, mixed batches, independence of the handle, injection against the seed, the refusal, the
serving layers the emulator can run (group, coalescer, streams, pool) and the host layers (PiperVoice, piper_amd.infer,
SynthesisConfig::seed through tests/cpp/test_seeds.cpp). tests/seeds_case.py holds what this file shares with
tests/test_gpu_seeds.py; the device's transcendental units, graphs and concurrent callers are that file's.

The emulator runs the vocoder slowly, so the cases are the smallest that reach each draw site: a few ids per utterance where
the whole call runs, and the first chunk of a batch stream (text encoder, durations, flow, one short window) where only the
duration noise matters -- which of embed_kernel / randn_kernel draws it is a matter of the id bucket alone."""
import io
import json
import os
import re
import subprocess

import ctypes as C
import numpy as np
import pytest

import one_utterance_truth_case as U
import rng_case as R
import seeds_case as S
from piper_amd import _lib as L, weights as W
from piper_amd.engine import Engine, EngineError

EMU = os.path.join(U.ROOT, "tests", "emu", "libpiper_hip_emu.so")
GATE = R.EMU_GATE


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", U.ROOT, "emu"])
    lib = L.bind(EMU)
    yield lib
    U.close_engines()


@pytest.fixture(scope="module")
def oracle(emu_lib):
    """The handle whose debug_randn gives the expected draws: the engines under test keep their own seed and counter."""
    return U.engine_for("tiny", {}, lib=emu_lib)


def _fresh(emu_lib, seed=None, name="tiny", env=None):
    eng = U.engine_for(name, env or {}, lib=emu_lib, fresh=True)
    if seed is not None:
        eng.set_seed(seed)
    return eng


@pytest.mark.parametrize("env", [{}, {"PIPER_HIP_IDS_ZC": 0}], ids=["zero-copy", "copied"])
def test_mixed_batch(emu_lib, oracle, env):
    """use = [1, 0, 1, 0], the keys read from the pinned block or copied with it: the seeded rows are their seeds' streams at
    counter 0, the others the engine's own at (engine seed, call, row = b * channels + c); two utterances with the same ids
    and the same seed are the same utterance."""
    cfg, _ = U.voice("tiny")
    lens = [6, 3, 6, 4]
    ids = S.ids_of(cfg, lens)
    ids[2] = ids[0]
    seeds = [S.SEEDS[4], None, S.SEEDS[4], None]
    eng = _fresh(emu_lib, 999, env=env)
    try:
        r = eng.synthesize_batch(ids, S.SCALES, seeds=seeds)
        assert eng.rng_calls == 1
        S.check_noise(eng, oracle, cfg, seeds, lens, GATE, "emu mixed", engine_seed=999, call=1)
        d = eng.durations()
        assert np.array_equal(eng.debug_tensor("noise_w", 0), eng.debug_tensor("noise_w", 2))
        assert np.array_equal(eng.debug_tensor("noise_z", 0), eng.debug_tensor("noise_z", 2))
        assert np.array_equal(d[:6], d[9:15]) and r.frames[0] == r.frames[2]
        assert np.array_equal(r.pcm[0], r.pcm[2])
        # the next call, unseeded, is the engine's own stream at the next counter: the seeds went with the upload
        eng.synthesize_batch(ids, S.SCALES)
        R.check_engine_noise(eng, cfg, 999, 2, lens, GATE, "emu unseeded after seeded")
    finally:
        eng.close()


@pytest.mark.parametrize("lens, drawn_by", [([128, 3, 1, 2], "embed_kernel"), ([129, 3, 1, 2], "randn_kernel")])
def test_duration_noise_on_both_sides_of_the_embed_seam(emu_lib, oracle, lens, drawn_by):
    """256 Philox blocks: embed_kernel's draw loop picks the key per block; one more id: a randn_kernel launch, the key per
    workgroup. First chunk of a batch stream, under the level-2 profile; utterance 1 keeps the engine's own stream."""
    cfg, _ = U.voice("tiny")
    ids = S.ids_of(cfg, lens)
    seeds = [S.SEEDS[1], None, S.SEEDS[0], S.SEEDS[2]]
    eng = _fresh(emu_lib, 31)
    try:
        def call():
            chunks = eng.stream_batch(ids, S.SCALES, chunk_frames=2, seeds=seeds)
            next(chunks)
            chunks.close()
        names = S.profiled_names(eng, call)
        S.check_noise(eng, oracle, cfg, seeds, lens, GATE, f"emu seam {lens[0]}", sites=(0,), engine_seed=31, call=1)
    finally:
        eng.close()
    assert ("randn_kernel" in names) == (drawn_by == "randn_kernel") and "embed_kernel" in names and "regulate_kernel" in names, names


def test_independent_of_the_handle_and_repeatable(emu_lib):
    """Two handles with other engine seeds, one of them with calls behind it: the same seeded call gives the same audio.
    pe_run twice on one seeded upload draws the same noise again while the run counter advances."""
    cfg, _ = U.voice("tiny")
    ids = S.ids_of(cfg, [7, 4])
    seeds = S.seeds_for(2, 3)
    a, b = _fresh(emu_lib, 1), _fresh(emu_lib, 999)
    try:
        b.synthesize_batch(S.ids_of(cfg, [5], first=3), S.SCALES)
        b.synthesize_batch(S.ids_of(cfg, [3, 3], first=9), S.SCALES, seeds=[5, None])
        ra, rb = a.synthesize_batch(ids, S.SCALES, seeds=seeds), b.synthesize_batch(ids, S.SCALES, seeds=seeds)
        assert (a.rng_calls, b.rng_calls) == (1, 3)
        for u in range(2):
            assert np.array_equal(ra.audio[u], rb.audio[u]) and np.array_equal(ra.pcm[u], rb.pcm[u]), u
        assert np.array_equal(ra.frames, rb.frames)
        plain = a.synthesize_batch(ids, S.SCALES)
        assert not np.array_equal(plain.frames, ra.frames) or not np.array_equal(plain.audio[0], ra.audio[0])
        a.upload(ids, S.SCALES, seeds=seeds)
        n0 = a.rng_calls
        a.run()
        r1 = a.fetch()
        a.run()
        r2 = a.fetch()
        assert a.rng_calls == n0 + 2
        for u in range(2):
            assert np.array_equal(r1.audio[u], r2.audio[u]) and np.array_equal(r1.pcm[u], ra.pcm[u]), u
    finally:
        a.close()
        b.close()


def test_injection_wins_at_its_site_and_equals_the_seed(emu_lib, oracle):
    """noise_w injected beside a seed: noise_w is the injected array, noise_z the seed's. Both sites injected from the
    seed's own draws: the seeded call again."""
    cfg, _ = U.voice("tiny")
    lens = [6]
    ids = S.ids_of(cfg, lens)
    seed = S.SEEDS[3]
    eng = _fresh(emu_lib, 5)
    try:
        base = eng.synthesize_batch(ids, S.SCALES, seeds=[seed])
        d0 = eng.durations()
        nw = np.random.default_rng(3).standard_normal((1, 2, 6)).astype(np.float32)
        eng.synthesize_batch(ids, S.SCALES, noise_w=nw, seeds=[seed])
        assert np.array_equal(eng.debug_tensor("noise_w", 0), nw[0])
        S.check_noise(eng, oracle, cfg, [seed], lens, GATE, "emu injected w", sites=(1,))
        F = int(base.frames[0])
        inj_w = S.expected(oracle, seed, 0, 0, 0, 2, 6)[None]
        inj_z = S.expected(oracle, seed, 0, 1, 0, cfg.inter, F)[None]
        r = eng.synthesize_batch(ids, S.SCALES, noise_w=inj_w, noise_z=inj_z)
        assert np.array_equal(eng.durations(), d0) and np.array_equal(r.frames, base.frames)
        S.pcm_close(r.pcm[0], base.pcm[0], "emu seed against injection")
    finally:
        eng.close()


def test_seeds_without_a_seed_array_are_refused(emu_lib):
    """A pe_seeds with a NULL seed: refused with a message, and the engine is as it was -- the next unseeded call draws the
    engine's own stream at the next counter."""
    cfg, _ = U.voice("tiny")
    lens = [5]
    ids = S.ids_of(cfg, lens)
    eng = _fresh(emu_lib, 77)
    try:
        eng.synthesize_batch(ids, S.SCALES)
        flat, offs = eng._pack(ids)
        sc = np.ascontiguousarray(np.tile(np.asarray(S.SCALES, np.float32), (1, 1)))
        bad = L.PeSeeds()
        res = L.PeResult()
        i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
        args = (eng._h, flat.ctypes.data_as(i64p), offs.ctypes.data_as(i64p), 1, sc.ctypes.data_as(f32p), None, None)
        assert emu_lib.pe_synthesize_batch_seeded(*args, C.byref(res), None, C.byref(bad)) != 0
        assert b"seed" in emu_lib.pe_last_error()
        assert emu_lib.pe_upload_seeded(*args, None, C.byref(bad)) != 0 and b"seed" in emu_lib.pe_last_error()
        assert eng.rng_calls == 1
        eng.synthesize_batch(ids, S.SCALES)
        R.check_engine_noise(eng, cfg, 77, 2, lens, GATE, "emu after the refusal")
        with pytest.raises(ValueError):
            eng.synthesize_batch(ids, S.SCALES, seeds=[1, 2])
    finally:
        eng.close()


def test_one_utterance_stream_and_pool(emu_lib, oracle):
    """A seeded one-utterance stream holds its seed's noise at both sites after the first chunk; a seeded newcomer of a
    stream pool has the durations of its seeded whole-utterance call."""
    cfg, _ = U.voice("tiny")
    ids = S.ids_of(cfg, [6, 5, 4])
    seed = S.SEEDS[4]
    eng = _fresh(emu_lib, 8)
    try:
        chunks = eng.stream(ids[0], S.SCALES, chunk_frames=4, seed=seed)
        next(chunks)
        frames = S.check_noise(eng, oracle, cfg, [seed], [6], GATE, "emu stream")
        chunks.close()
        assert frames[0] == eng.stream_frames
        whole = eng.synthesize_batch([ids[0]], S.SCALES, seeds=[seed])
        d = eng.durations()
        assert int(whole.frames[0]) == frames[0]
        with eng.stream_pool(3, 256) as pool:
            pool.join(ids[1:], S.SCALES)
            pool.next(4)
            slot = pool.join([ids[0]], S.SCALES, seeds=[seed])[0]
            assert np.array_equal(eng.durations(), d)
            got = []
            while True:
                out = pool.next(8)
                if not out:
                    break
                if slot in out:
                    got.append(out[slot][0])
            a = np.concatenate(got)
            assert a.size == whole.audio[0].size
            err = float(np.max(np.abs(a - whole.audio[0])))
            print(f"[emu pool] seeded newcomer against its whole call: max |d| {err:.3e}")
            assert err < 2e-4          # (tests/test_gpu_stream_pool.py: a slot's chunks against the whole call)
    finally:
        eng.close()


def test_group_and_coalescer(emu_lib, oracle, monkeypatch):
    """A group of two members, both taking part: each member's utterance holds its seed's noise, and the result is one
    engine's seeded call in the caller's order. A coalesced seeded request is its own seeded B = 1 call."""
    from piper_amd.group import Coalescer, EngineGroup
    cfg, w = U.voice("tiny")
    blob = W.pack_blob(cfg, w)
    lens = [7, 5]
    ids = S.ids_of(cfg, lens)
    seeds = S.seeds_for(2, 1)
    monkeypatch.setenv("PIPER_HIP_GROUP_COALESCE", "0")
    monkeypatch.setenv("PIPER_HIP_DEBUG_KEEP", "1")
    grp = EngineGroup(blob, [0, 0], lib=emu_lib)
    eng = _fresh(emu_lib, 4)
    try:
        r = grp.synthesize_batch(ids, S.SCALES, seeds=seeds)
        assign = grp.assignment(2)
        assert sorted(assign) == [0, 1]
        for u in range(2):
            S.check_noise(grp.engine(assign[u]), oracle, cfg, [seeds[u]], [lens[u]], GATE, f"emu group utt {u}")
        one = eng.synthesize_batch(ids, S.SCALES, seeds=seeds)
        for u in range(2):
            assert r.frames[u] == one.frames[u]
            S.pcm_close(r.pcm[u], one.pcm[u], f"emu group utt {u}")
        co = Coalescer(eng, max_batch=4, mix_scales=True)
        try:
            pcm, frames, _, _ = co.synthesize(ids[0], S.SCALES, seed=seeds[0])
            assert frames == one.frames[0]
            S.pcm_close(pcm, one.pcm[0], "emu coalescer")
            before = eng.rng_calls
            co.synthesize(ids[0], S.SCALES)
            R.check_engine_noise(eng, cfg, 4, before + 1, [lens[0]], GATE, "emu coalescer unseeded")
        finally:
            co.close()
    finally:
        grp.close()
        eng.close()


def test_voice_and_driver(emu_lib, tmp_path, monkeypatch):
    """PiperVoice(seed=) repeats itself; piper_amd.infer --seed N gives line k the seed N + k and a line's own "seed"
    overrides it, whatever --batch: the seeds that reach Engine.synthesize_batch, and WAVs that do not depend on --batch."""
    import wave
    from piper_amd import infer
    from piper_amd.config import PiperConfig
    from piper_amd.voice import PiperVoice
    model = os.path.join(U.ROOT, "tests", "golden", "tiny_voice.onnx")
    conf = PiperConfig.from_dict(json.load(open(model + ".json", encoding="utf-8")))
    voice = PiperVoice(session=Engine(onnx_path=model, lib=emu_lib), config=conf)
    ids = [int(x) for x in W.synthetic_phoneme_ids(7, 3, id_max=39)]
    a = voice.synthesize_ids_to_raw(ids, seed=11)
    voice.synthesize_ids_to_raw(ids)
    assert voice.synthesize_ids_to_raw(ids, seed=11) == a != voice.synthesize_ids_to_raw(ids, seed=12)
    two = voice.synthesize_ids_batch_to_raw([ids[:4], ids], seeds=[None, 11])
    assert two[1] == a
    voice.session.close()

    assert infer.read_seeds(['{"phoneme_ids": [1]}', "", '{"phoneme_ids": [1], "seed": 5}', '{"phoneme_ids": [2]}'], 2 ** 64 - 2) == \
        [2 ** 64 - 2, 5, 1]
    assert infer.read_seeds(['{"phoneme_ids": [1]}', '{"phoneme_ids": [1], "seed": -1}'], None) == [None, 2 ** 64 - 1]
    seen = []
    real = Engine.synthesize_batch

    def spy(self, id_lists, scales=(0.667, 1.0, 0.8), **kw):
        seen.append(kw.get("seeds"))
        return real(self, id_lists, scales, **kw)
    monkeypatch.setattr(Engine, "synthesize_batch", spy)
    lines = [json.dumps({"phoneme_ids": ids}), "", json.dumps({"phoneme_ids": ids[:5], "seed": 40}), json.dumps({"phoneme_ids": ids})]
    wavs = {}
    for batch in (1, 2):
        out = tmp_path / f"wavs{batch}"
        seen.clear()
        assert infer.main(["--model", model, "--output-dir", str(out), "--sample-rate", "16000", "--batch", str(batch), "--seed", "7"],
                          stdin=io.StringIO("\n".join(lines)), lib=emu_lib) == 0
        assert [s for call in seen for s in call] == [7, 40, 10], seen
        for k in (0, 2, 3):
            with wave.open(str(out / f"{k}.wav"), "rb") as wv:
                wavs[batch, k] = wv.readframes(wv.getnframes())
    for k in (0, 2, 3):
        assert wavs[1, k] == wavs[2, k], k
    seen.clear()
    assert infer.main(["--model", model, "--output-dir", str(tmp_path / "plain")], stdin=io.StringIO(lines[0]), lib=emu_lib) == 0
    assert seen == [None]


def test_synthesis_config_seed_through_piper_hpp():
    """tests/cpp/test_seeds.cpp against the emulator build: phrase k of textToAudio draws from seed + k, wrapping."""
    exe = os.path.join(U.ROOT, "tests", "cpp", "test_seeds_emu")
    deps = [EMU, os.path.join(U.ROOT, "tests", "cpp", "test_seeds.cpp"), os.path.join(U.ROOT, "include", "piper.hpp"),
            os.path.join(U.ROOT, "include", "piper_hip.h")]
    if not all(os.path.exists(f) for f in [exe] + deps) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["make", "-C", U.ROOT, "emu", "tests/cpp/test_seeds_emu"], stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, os.path.join(U.ROOT, "tests", "golden", "tiny_voice.onnx")], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, PIPER_HIP_DEBUG_KEEP="1"))
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"^phrase (\d) ids=(\d+) seed=(\d+) match=(\d) next=(\d)", out.stdout, re.M)
    assert [(int(k), int(s)) for k, _, s, _, _ in rows] == [(0, 2 ** 64 - 1), (1, 0), (2, 1)]
    assert all(m == "1" and nx == "0" for _, _, _, m, nx in rows)
    assert len(re.findall(r"^utterance \d ids=\d+ seed=10\d match=1", out.stdout, re.M)) == 2
    assert re.search(r"^OK phrases=3 law=1 one=1 repeat=1 plain_differs=1 other_seed_differs=1", out.stdout, re.M)
