"""Output-rate conversion on the MI355X (run with -m gpu): the cases of tests/test_resample_emu.py on the device -- the kernel
against the f64 truth, whole utterances (also under PIPER_HIP_MATRIX=f16x3, whose generator tail differs), the three kinds
of streams, the untouched native rate with captured graphs -- and, at 8000 Hz, a coalescer of four threads, an engine group
on devices [0, 0] and one utterance of the full medium voice. The bound of every pointwise comparison is the a-priori one
of tests/resample_case.py."""
import json
import os
import sys
import threading

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import resample_case as R                                # noqa: E402
import stream_batch_case as K                            # noqa: E402
import test_resample_emu as E                            # noqa: E402

pytestmark = pytest.mark.gpu


def _clean_env(monkeypatch, env=None):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))


@pytest.mark.parametrize("fs_in", [16000, 22050])
def test_kernel_against_f64_truth(monkeypatch, fs_in):
    """Cases 1 and 3: ragged noise rows for every rate pair, and outputs from index 33 000 000 on at 22050 -> 48000."""
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib(), fs_in)
    for a, b in E.PAIRS:
        if a == fs_in:
            eng.set_output_rate(b)
            E.noise_rows(eng, a, b)
    if fs_in == 22050:
        eng.set_output_rate(48000)
        E.large_indices(eng)
    eng.close()


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_whole_utterances(monkeypatch, mode):
    """Case 4 on poisoned workspaces, in the f32 engine and in matrix mode f16x3 (read at engine creation)."""
    _clean_env(monkeypatch, dict({"PIPER_HIP_DEBUG_POISON": 1}, **({} if mode == "f32" else {"PIPER_HIP_MATRIX": mode})))
    cfg, _, eng = E._engine(L.get_lib())
    ids, nw, nz = K.inputs(cfg)
    native = eng.synthesize_batch(ids, K.SCALES, noise_w=nw, noise_z=nz)
    durations = eng.durations()
    for rate in (8000, 48000):
        E.whole_utterances(eng, cfg, rate, native, durations)
    eng.close()


@pytest.mark.parametrize("rate", [8000, 48000])
def test_streams(monkeypatch, rate):
    """Case 5: the one-utterance and the lock-step stream on the tiny voice, the pool scenario on the multi-speaker tiny-high
    voice, where the slot the fourth text reuses had a tenant with another speaker."""
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = E._engine(L.get_lib())
    E.one_streams(eng, cfg, rate)
    E.lock_step(eng, cfg, rate)
    eng.close()
    cfg, _, eng = E._engine(L.get_lib(), preset="tiny-high-ms")
    E.pool(eng, cfg, rate, multi_speaker=True)
    eng.close()


def test_native_rate_is_untouched(monkeypatch):
    """Case 6 with captured graphs: the one-utterance call is the speculative one-graph form."""
    _clean_env(monkeypatch)
    E.nothing_else_moved(lambda: E._engine(L.get_lib()), graphs=True)


def _as_case_4(eng, res, fs_in, rate, what):
    """The rows of the engine's last call: floats against the f64 resampling of the call's native waveform, int16 = the
    conversion of the floats, lengths ceil(S L / M)."""
    from oracle import vits_oracle as O
    for b in range(len(res.pcm)):
        x = eng.debug_tensor("audio", b)[0]
        assert x.size == int(res.frames[b]) * eng.hop
        assert res.audio[b].size == res.pcm[b].size == R.n_out(x.size, fs_in, rate), (what, b)
        want, bound = R.truth(x, fs_in, rate)
        R.assert_within(res.audio[b], want, bound, f"{what}, row {b}")
        assert np.array_equal(O.audio_float_to_int16(res.audio[b]), res.pcm[b]), (what, b)


def test_coalescer_and_group_at_8000(monkeypatch):
    """Four caller threads on a coalescer and an engine group on devices [0, 0], the engines at 8000 Hz: every request's
    pcm has ceil(S L / M) samples; the engine calls behind them are checked like case 4 (float rows against the f64
    resampling of that call's native waveform, the delivered int16 = the conversion of those floats)."""
    from piper_amd.group import Coalescer, EngineGroup
    _clean_env(monkeypatch)
    cfg, w, eng = E._engine(L.get_lib())
    fs_in, rate, hop = cfg.sample_rate, 8000, eng.hop
    ids = [W.synthetic_phoneme_ids(T, 300 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate((9, 17, 12, 23))]
    zero = (0.0, 1.0, 0.0)                               # no noise: a request is what its own call computes
    eng.set_output_rate(rate)
    alone = []
    for t in ids:
        r = eng.synthesize(t, zero)
        _as_case_4(eng, r, fs_in, rate, f"one call of {len(t)} ids")
        alone.append(r)
    co = Coalescer(eng, max_batch=4, max_wait_us=200000)
    out = [None] * 4

    def work(i):
        out[i] = co.synthesize(ids[i], zero)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    calls, reqs = co.stats
    last = eng.fetch(True, True)                         # the rows of the last engine call the coalescer made
    _as_case_4(eng, last, fs_in, rate, "the coalescer's last engine call")
    served = 0
    for i in range(4):
        pcm, frames, _, _ = out[i]
        assert frames == int(alone[i].frames[0]) and pcm.size == R.n_out(frames * hop, fs_in, rate), i
        assert np.max(np.abs(pcm.astype(np.int32) - alone[i].pcm[0].astype(np.int32))) <= 2, i      # (another batch size)
        served += any(p.size == pcm.size and np.array_equal(p, pcm) for p in last.pcm)
    assert reqs == 4 and served == len(last.pcm), (calls, reqs, served)
    print(f"coalescer: 4 requests in {calls} engine calls, the last one of {len(last.pcm)}")
    co.close()
    eng.close()
    grp = EngineGroup(W.pack_blob(cfg, w), [0, 0])
    members = [grp.engine(i) for i in range(len(grp))]
    for m in members:
        m.set_output_rate(rate)
    grp.set_seed(11)
    r = grp.synthesize_batch(ids, zero)
    who = grp.assignment(4)
    for i, m in enumerate(members):
        mine = [u for u in range(4) if who[u] == i]
        if not mine:
            continue
        res = m.fetch(True, True)
        _as_case_4(m, res, fs_in, rate, f"group engine {i}")
        assert sorted(p.size for p in res.pcm) == sorted(r.pcm[u].size for u in mine)
        for u in mine:
            assert any(p.size == r.pcm[u].size and np.array_equal(p, r.pcm[u]) for p in res.pcm), u
    for u in range(4):
        assert int(r.frames[u]) == int(alone[u].frames[0]) and r.pcm[u].size == R.n_out(int(r.frames[u]) * hop, fs_in, rate)
    for m in members:
        m.close()
    grp.close()


def test_full_medium_voice(monkeypatch, tmp_path):
    """One 40-id utterance of the full-size medium voice (an .onnx: the native rate comes from the caller) at 48000 and at
    8000 Hz, checked like case 4."""
    from oracle import voice_skeleton as S
    from piper_amd.engine import Engine
    _clean_env(monkeypatch)
    eng = Engine(onnx_path=S.fill("medium_voice.onnx", str(tmp_path)), device=0)
    assert eng.sample_rate == 0
    ids = W.synthetic_phoneme_ids(40, 7, id_max=min(eng.num_symbols - 1, 129))
    rng = np.random.default_rng(40)
    nw = rng.standard_normal((2, 40)).astype(np.float32)
    nz = rng.standard_normal((192, 6 * 40 + 64)).astype(np.float32)
    native = eng.synthesize(ids, (0.667, 1.0, 0.8), noise_w=nw, noise_z=nz)
    for rate in (48000, 8000):
        eng.set_output_rate(rate, native=22050)
        assert eng.resample_half_width == R.params(22050, rate).K
        r = eng.synthesize(ids, (0.667, 1.0, 0.8), noise_w=nw, noise_z=nz)
        assert np.array_equal(r.frames, native.frames)
        _as_case_4(eng, r, 22050, rate, f"medium voice, 22050->{rate}")
    eng.close()


def test_piper_voice_output_sample_rate(monkeypatch):
    """PiperVoice.load(..., output_sample_rate=): the config's rate is passed as the native one (an .onnx has none), the
    delivered audio has ceil(S L / M) samples and `sample_rate` -- what the WAV header and the silences use -- is the new rate."""
    from piper_amd.voice import PiperVoice
    _clean_env(monkeypatch)
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    plain = PiperVoice.load(model)
    voice = PiperVoice.load(model, output_sample_rate=8000)
    native = plain.config.sample_rate
    assert plain.sample_rate == native and voice.sample_rate == 8000 and voice.session.native_rate == native
    ids = [int(v) for v in W.synthetic_phoneme_ids(9, 3, id_max=39)]
    a = plain.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0)
    b = voice.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0)
    assert len(b) // 2 == R.n_out(len(a) // 2, native, 8000) and len(b) > 0
    plain.session.close()
    voice.session.close()


@pytest.mark.parametrize("rate", [0, 8000, 48000])
def test_missed_guess(monkeypatch, rate):
    """A speculative call whose guess was too small, at the native rate and at a converted one (tests/test_resample_emu.py)."""
    _clean_env(monkeypatch)
    cfg, _, eng = E._engine(L.get_lib())
    E.missed_guess(eng, cfg, rate)
    eng.close()
