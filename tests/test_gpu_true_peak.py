"""The true-peak ceiling of the target loudness on the MI355X (run with -m gpu): the cases of tests/test_true_peak_emu.py
on the device -- the interpolator's table, the kernel against the f64 truth, whole utterances with both kinds of ceiling on
poisoned workspaces (also under PIPER_HIP_MATRIX=f16x3), the speculative one-graph form with captured graphs, the untouched
sample-peak kind, the refusals -- and an engine group on devices [0, 0], PiperVoice.load(true_peak=) and the command-line
tool."""
import json
import os
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import loudness_case as LC                               # noqa: E402
import test_loudness_emu as E                            # noqa: E402
import test_true_peak_emu as T                           # noqa: E402
import true_peak_case as TP                              # noqa: E402

pytestmark = pytest.mark.gpu


def _clean_env(monkeypatch, env=None):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))


def test_filter(monkeypatch):
    _clean_env(monkeypatch)
    T.filter_table(L.get_lib())


@pytest.mark.parametrize("fs", TP.RATES)
def test_kernel_against_f64_truth(monkeypatch, fs):
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib())
    TP.check_kernel(eng, fs)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000, 48000])
def test_whole_utterances(monkeypatch, rate):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = E._engine(L.get_lib())
    T.whole_utterances(eng, cfg, rate)
    eng.close()


def test_whole_utterances_f16x3(monkeypatch):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1, "PIPER_HIP_MATRIX": "f16x3"})
    cfg, _, eng = E._engine(L.get_lib())
    T.whole_utterances(eng, cfg, 0)
    eng.close()


def test_speculative_form(monkeypatch):
    """With captured graphs: after pe_warmup every call replays the one graph, one launch more than with the sample-peak
    kind, and switching kinds captures nothing once each has been seen."""
    _clean_env(monkeypatch)
    T.speculative(lambda: E._engine(L.get_lib()), graphs=True)


def test_sample_is_the_parent(monkeypatch):
    _clean_env(monkeypatch)
    T.sample_is_parent(lambda: E._engine(L.get_lib()))


def test_refusals(monkeypatch):
    from piper_amd.engine import Engine
    _clean_env(monkeypatch)
    cfg, _, eng = E._engine(L.get_lib())
    T.refusals(eng, cfg, lambda: Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), device=0))
    eng.close()


def test_group_voice_and_infer(monkeypatch, tmp_path):
    """EngineGroup.set_loudness(true_peak=True) on devices [0, 0]: every member's call is checked like the whole
    utterances. PiperVoice.load(..., true_peak=True) sets the engine, and what it delivers obeys the ceiling as a true
    peak. piper_amd.infer --true-peak writes WAVs that do."""
    from piper_amd.group import EngineGroup
    from piper_amd.voice import PiperVoice
    _clean_env(monkeypatch)
    cfg, w, _eng = E._engine(L.get_lib())
    _eng.close()
    fs = cfg.sample_rate
    ids = [W.synthetic_phoneme_ids(n, 300 + i, id_max=cfg.n_vocab - 1) for i, n in enumerate((19, 27, 22, 33))]
    zero = (0.0, 2.0, 0.0)
    grp = EngineGroup(W.pack_blob(cfg, w), [0, 0])
    members = [grp.engine(i) for i in range(len(grp))]
    grp.set_loudness(-8.0, -1.0, true_peak=True)
    assert all(m.loudness() == (-8.0, -1.0) and m.loudness_ceiling() == (TP.TRUE, TP.oversample(fs), TP.K) for m in members)
    grp.set_seed(11)
    r = grp.synthesize_batch(ids, zero)
    who = grp.assignment(4)
    for i, m in enumerate(members):
        mine = [u for u in range(4) if who[u] == i]
        if not mine:
            continue
        res = m.fetch(True, True)
        TP.check_delivery(m, res, fs, -8.0, -1.0, f"group engine {i}: ")
        for u in mine:
            assert any(p.size == r.pcm[u].size and np.array_equal(p, r.pcm[u]) for p in res.pcm), u
    for m in members:
        m.close()
    grp.close()

    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    voice = PiperVoice.load(model, target_lufs=-5.0, peak_ceiling_db=-3.0, true_peak=True)
    rate = voice.config.sample_rate
    assert voice.session.loudness() == (-5.0, -3.0)
    assert voice.session.loudness_ceiling() == (TP.TRUE, TP.oversample(rate), TP.K)
    raw = voice.synthesize_ids_to_raw([int(v) for v in W.synthetic_phoneme_ids(30, 3, id_max=39)], noise_scale=0.0,
                                      noise_w=0.0, length_scale=2.0)
    pcm = np.frombuffer(raw, np.int16)
    tp = voice.session.last_true_peak()
    _, scale, peak, flags = voice.session.last_loudness()
    delivered = TP.true_peak(pcm.astype(np.float64) / 32767.0, rate)[0]
    C, S = 10.0 ** (-3.0 / 20.0), TP.truncation_slack(rate)
    print(f"PiperVoice: t {float(tp[0]):.6f}, p {float(peak[0]):.6f}, scale {float(scale[0]):.3f}, flags {int(flags[0])}, "
          f"delivered true peak {delivered:.5f} (ceiling {C:.5f})")
    assert tp.size == 1 and pcm.size > 0 and flags[0] & LC.LIMITED
    assert delivered <= C + S / 32767.0
    assert float(scale[0]) * max(float(tp[0]), float(peak[0])) <= 32767.0 * C
    voice.session.close()
    T.infer_true_peak(L.get_lib(), tmp_path)
