"""GPU checks of the kernels whose entry sequence takes leading scalar parameters (pe_rt.h PE_ENTRY_BATCH): every such
kernel, and every pointer among those parameters that may be null, runs once and the result is compared with the CPU
oracle at the tolerances of tests/test_gpu_parity.py -- integer durations equal, max |d audio| < 2e-4, int16 RMS <= 1e-3.

The lengths: 3 ids = a single partial 4-column tile; 5 = the half-group gate form; 64 / 128 / 129 = the id-bucket edge
and, at 129, attn4_kernel<96, true>. The x-low and tiny families run the generator / conv kernels on other channel
counts; the 4-column text-encoder and flow kernels (attn4, colchain4, lngemm4, ffn, dds_layer4, gate4) exist for
192-channel voices only, so the medium family runs the edge lengths as well."""
import numpy as np
import pytest

from piper_amd import weights as W

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3           # as tests/test_gpu_parity.py
TIGHT_AUDIO_TOL = 2e-4
SCALES = (0.667, 1.0, 0.8)

_engines = {}


def engine_for(preset, seed=1234):
    from piper_amd.engine import Engine
    if preset not in _engines:
        cfg = W.preset(preset)
        w = W.synthetic_weights(cfg, seed)
        _engines[preset] = (cfg, w, Engine(blob=W.pack_blob(cfg, w), device=0))
    return _engines[preset]


def noise_for(cfg, T, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((2, T)).astype(np.float32), rng.standard_normal((cfg.inter, 32 * T + 64)).astype(np.float32)


def pcm_rms(a, b):
    d = (a.astype(np.float64) - b.astype(np.float64)) / 32767.0
    return float(np.sqrt(np.mean(d * d))) if d.size else 0.0


def check(audio, pcm, o):
    assert audio.shape == o["audio"].shape
    assert np.max(np.abs(audio - o["audio"])) < TIGHT_AUDIO_TOL
    assert pcm_rms(pcm, o["pcm"]) <= RMS_TOL


@pytest.mark.parametrize("preset,T", [(p, T) for p in ("x-low", "tiny") for T in (3, 5, 64, 128, 129)] +
                         [("medium", 3), ("medium", 5), ("medium", 129)])
def test_one_utterance(preset, T):
    from oracle import vits_oracle as O
    cfg, w, eng = engine_for(preset)
    ids = W.synthetic_phoneme_ids(T, 3, id_max=min(cfg.n_vocab - 1, 129))
    nw, nz = noise_for(cfg, T, 100 + T)
    o = O.synthesize(w, cfg, ids, SCALES, nw, nz)
    r = eng.synthesize(ids, SCALES, noise_w=nw, noise_z=nz)
    assert np.array_equal(eng.durations(), o["durations"])
    check(r.audio[0], r.pcm[0], o)


@pytest.mark.parametrize("preset", ["x-low", "medium"])
def test_two_ragged_utterances(preset):
    """7 and 128 ids in one call: ragged lengths, the utterance index on blockIdx.y / blockIdx.z."""
    from oracle import vits_oracle as O
    cfg, w, eng = engine_for(preset)
    Ts = [7, 128]
    id_lists = [W.synthetic_phoneme_ids(T, i, id_max=min(cfg.n_vocab - 1, 129)) for i, T in enumerate(Ts)]
    rng = np.random.default_rng(31)
    nw = rng.standard_normal((2, 2, max(Ts))).astype(np.float32)
    nz = rng.standard_normal((2, cfg.inter, 32 * max(Ts) + 64)).astype(np.float32)
    rb = eng.synthesize_batch(id_lists, SCALES, noise_w=nw, noise_z=nz)
    durs = eng.durations()
    off = 0
    for i, ids in enumerate(id_lists):
        o = O.synthesize(w, cfg, ids, SCALES, nw[i], nz[i])
        assert np.array_equal(durs[off:off + len(ids)], o["durations"])
        off += len(ids)
        check(rb.audio[i], rb.pcm[i], o)


def test_multi_speaker_conditioning_pointers():
    """the multi-speaker tiny voice at 33 ids: the per-utterance conditioning biases are non-null"""
    from oracle import vits_oracle as O
    cfg, w, eng = engine_for("tiny-ms")
    T = 33
    ids = W.synthetic_phoneme_ids(T, 2, id_max=cfg.n_vocab - 1)
    nw, nz = noise_for(cfg, T, 53)
    o = O.synthesize(w, cfg, ids, SCALES, nw, nz, sid=2)
    r = eng.synthesize(ids, SCALES, sid=2, noise_w=nw, noise_z=nz)
    assert np.array_equal(eng.durations(), o["durations"])
    check(r.audio[0], r.pcm[0], o)


@pytest.mark.parametrize("preset,T,chunk", [("x-low", 24, 45), ("medium", 24, 45)])
def test_streaming_window(preset, T, chunk):
    """the generator kernels on a stream window's own length pointer, against the oracle's chunked decode"""
    from oracle import vits_oracle as O
    cfg, w, eng = engine_for(preset)
    ids = W.synthetic_phoneme_ids(T, 5, id_max=min(cfg.n_vocab - 1, 129))
    nw, nz = noise_for(cfg, T, 13)
    o = O.synthesize(w, cfg, ids, SCALES, nw, nz, keep=True)
    chunks = list(eng.stream(ids, SCALES, chunk_frames=chunk, noise_w=nw, noise_z=nz))
    assert eng.stream_frames == o["frames"]
    ref = O.stream_chunks(w, cfg, o["z"], chunk, eng.stream_halo)
    assert len(ref) == len(chunks)
    for (a, p), (ra, rp) in zip(chunks, ref):
        assert a.shape == ra.shape and p.shape == rp.shape
        assert np.max(np.abs(a - ra)) < TIGHT_AUDIO_TOL
        assert pcm_rms(p, rp) <= RMS_TOL
