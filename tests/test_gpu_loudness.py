"""Target loudness on the MI355X (run with -m gpu): the cases of tests/test_loudness_emu.py on the device -- the kernels
against the f64 truth (and one row of 30 s at 48000 Hz), whole utterances on poisoned workspaces (also under
PIPER_HIP_MATRIX=f16x3), the speculative one-graph form with captured graphs, the untouched default and streams -- and a
coalescer of four threads, an engine group on devices [0, 0], one utterance of the full medium voice at 22050 and 8000 Hz,
PiperVoice.load(target_lufs=) and the command-line tool."""
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
import loudness_case as LC                               # noqa: E402
import test_loudness_emu as E                            # noqa: E402

pytestmark = pytest.mark.gpu


def _clean_env(monkeypatch, env=None):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))


def test_coefficients(monkeypatch):
    _clean_env(monkeypatch)
    E.test_coefficients(L.get_lib())


@pytest.mark.parametrize("fs", LC.RATES)
def test_kernel_against_f64_truth(monkeypatch, fs):
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib())
    LC.check_kernel(eng, fs)
    eng.close()


def test_kernel_thirty_seconds(monkeypatch):
    """One row of 30 s at 48000 Hz: 300 segments, 297 blocks; the bursts repeated every 1.3 s, so both gates keep dropping."""
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib())
    fs, h = 48000, 4800
    one = LC.bursts(13 * h, fs, 77)
    x = np.tile(one, 30 * fs // one.size + 1)[:30 * fs]
    res = LC.check_rows(eng, fs, [("thirty", x), ("tail", x[:7 * h + 11])])
    t = res["thirty"][0]
    assert t.dropped_abs >= 20 and t.dropped_rel >= 20, (t.dropped_abs, t.dropped_rel)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000, 48000])
def test_whole_utterances(monkeypatch, rate):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = E._engine(L.get_lib())
    E.whole_utterances(eng, cfg, rate)
    eng.close()


def test_whole_utterances_f16x3(monkeypatch):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1, "PIPER_HIP_MATRIX": "f16x3"})
    cfg, _, eng = E._engine(L.get_lib())
    E.whole_utterances(eng, cfg, 0)
    eng.close()


def test_speculative_form(monkeypatch):
    """With captured graphs: after pe_warmup every call replays the one graph, and new T / C values capture nothing."""
    _clean_env(monkeypatch)
    E.speculative(lambda: E._engine(L.get_lib()), graphs=True)


def test_off_is_the_parent(monkeypatch):
    _clean_env(monkeypatch)
    E.off_is_parent(lambda: E._engine(L.get_lib()))


def test_streams_untouched(monkeypatch):
    """The streams of the tiny voice, and the pool scenario on the multi-speaker tiny-high voice."""
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = E._engine(L.get_lib())
    pcfg, _, peng = E._engine(L.get_lib(), preset="tiny-high-ms")
    E.streams_untouched(eng, cfg, peng, pcfg, multi_speaker=True)
    eng.close()
    peng.close()


def test_refusals(monkeypatch):
    _clean_env(monkeypatch)
    cfg, _, eng = E._engine(L.get_lib())
    E.refusals(eng, cfg)
    eng.close()


def test_coalescer_and_group(monkeypatch):
    """Four caller threads on a coalescer and an engine group on devices [0, 0], every engine at -20 LUFS: the engine calls
    behind them are checked like the whole utterances (report against the f64 loudness of the call's floats, int16 = the
    conversion with the reported scale), and every request's pcm is one of those rows."""
    from piper_amd.group import Coalescer, EngineGroup
    _clean_env(monkeypatch)
    cfg, w, eng = E._engine(L.get_lib())
    fs = cfg.sample_rate
    ids = [W.synthetic_phoneme_ids(T, 300 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate((19, 27, 22, 33))]
    zero = (0.0, 2.0, 0.0)                               # no noise: a request is what its own call computes
    eng.set_loudness(-20.0, -1.0)
    co = Coalescer(eng, max_batch=4, max_wait_us=200000)
    out = [None] * 4

    def work(i):
        out[i] = co.synthesize(ids[i], zero)

    th = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    calls, reqs = co.stats
    last = eng.fetch(True, True)
    LC.check_delivery(eng, last, fs, -20.0, -1.0, "the coalescer's last engine call: ")
    served = sum(any(p.size == out[i][0].size and np.array_equal(p, out[i][0]) for p in last.pcm) for i in range(4))
    assert reqs == 4 and served == len(last.pcm), (calls, reqs, served)
    for i in range(4):
        pcm = out[i][0]
        t = LC.Truth(pcm.astype(np.float64) / 32767.0, fs)
        peak = int(np.max(np.abs(pcm.astype(np.int32))))
        print(f"request {i}: {pcm.size} samples, {t.L:.4f} LUFS, peak {peak}")
        ceil = 32767.0 * 10.0 ** (-1.0 / 20.0)
        assert peak <= ceil
        # at the target, unless short or held by the ceiling (truncation toward zero: tests/test_loudness_emu.py, infer_target_lufs)
        assert t.flags & LC.SHORT or peak >= int(ceil) - 1 or abs(t.L + 20.0) <= 0.01, (i, t.L, peak)
    co.close()
    eng.close()
    grp = EngineGroup(W.pack_blob(cfg, w), [0, 0])
    members = [grp.engine(i) for i in range(len(grp))]
    grp.set_loudness(-20.0, -1.0)
    assert all(m.loudness() == (-20.0, -1.0) for m in members)
    grp.set_seed(11)
    r = grp.synthesize_batch(ids, zero)
    who = grp.assignment(4)
    for i, m in enumerate(members):
        mine = [u for u in range(4) if who[u] == i]
        if not mine:
            continue
        res = m.fetch(True, True)
        LC.check_delivery(m, res, fs, -20.0, -1.0, f"group engine {i}: ")
        for u in mine:
            assert any(p.size == r.pcm[u].size and np.array_equal(p, r.pcm[u]) for p in res.pcm), u
    for m in members:
        m.close()
    grp.close()


def test_full_medium_voice(monkeypatch, tmp_path):
    """One 40-id utterance of the full-size medium voice (an .onnx: the native rate comes from the caller) at 22050 and at
    8000 Hz."""
    from oracle import voice_skeleton as S
    from piper_amd.engine import Engine
    _clean_env(monkeypatch)
    eng = Engine(onnx_path=S.fill("medium_voice.onnx", str(tmp_path)), device=0)
    ids = W.synthetic_phoneme_ids(40, 7, id_max=min(eng.num_symbols - 1, 129))
    rng = np.random.default_rng(40)
    nw = rng.standard_normal((2, 40)).astype(np.float32)
    nz = rng.standard_normal((192, 6 * 40 + 64)).astype(np.float32)
    for rate in (22050, 8000):
        eng.set_output_rate(rate, native=22050)
        eng.set_loudness(None)
        off = eng.synthesize(ids, (0.667, 1.0, 0.8), noise_w=nw, noise_z=nz)
        eng.set_loudness(-19.0, -1.0)
        on = eng.synthesize(ids, (0.667, 1.0, 0.8), noise_w=nw, noise_z=nz)
        assert np.array_equal(on.audio[0].view(np.int32), off.audio[0].view(np.int32))
        LC.check_delivery(eng, on, rate, -19.0, -1.0, f"medium voice at {rate}: ")
    eng.close()


def test_piper_voice_and_infer(monkeypatch, tmp_path):
    """PiperVoice.load(..., target_lufs=, peak_ceiling_db=) sets the engine (the config's rate as the native one), and
    piper_amd.infer --target-lufs writes WAVs at the target."""
    from piper_amd.voice import PiperVoice
    _clean_env(monkeypatch)
    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    voice = PiperVoice.load(model, target_lufs=-18.0, peak_ceiling_db=-2.0)
    assert voice.session.loudness() == (-18.0, -2.0) and voice.session.native_rate == voice.config.sample_rate
    ids = [int(v) for v in W.synthetic_phoneme_ids(30, 3, id_max=39)]
    raw = voice.synthesize_ids_to_raw(ids, noise_scale=0.0, noise_w=0.0, length_scale=2.0)
    pcm = np.frombuffer(raw, np.int16)
    Lr, scale, peak, flags = voice.session.last_loudness()
    assert Lr.size == 1 and pcm.size > 0
    assert abs(int(np.max(np.abs(pcm.astype(np.int32)))) - float(peak[0]) * float(scale[0])) <= 1.0
    if not flags[0] & (LC.LIMITED | LC.UNMEASURABLE | LC.SHORT):
        assert abs(float(Lr[0]) + 20.0 * np.log10(float(scale[0]) / 32767.0) + 18.0) <= 1e-3
    voice.session.close()
    E.infer_target_lufs(L.get_lib(), tmp_path)
