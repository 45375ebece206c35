"""The look-ahead limiter of the target loudness on the MI355X (run with -m gpu): the cases of tests/test_limiter_emu.py on the
device -- the window, the kernel against the f64 truth, whole utterances on poisoned workspaces (also under
PIPER_HIP_MATRIX=f16x3), the clicks row, the speculative one-graph form with captured graphs, the untouched limiter-off
path, the refusals -- and an engine group on devices [0, 0], PiperVoice.load(limiter=) and the command-line tool."""
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
import limiter_case as LM                                # noqa: E402
import loudness_case as LC                               # noqa: E402
import test_limiter_emu as T                             # noqa: E402
import test_loudness_emu as E                            # noqa: E402

pytestmark = pytest.mark.gpu


def _clean_env(monkeypatch, env=None):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))


def test_window(monkeypatch):
    _clean_env(monkeypatch)
    T.window_table(L.get_lib())


@pytest.mark.parametrize("ms", LM.WINDOWS)
@pytest.mark.parametrize("fs", LM.RATES)
def test_kernel_against_f64_truth(monkeypatch, fs, ms):
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib())
    LM.check_kernel(eng, fs, ms)
    eng.close()


@pytest.mark.parametrize("ms", LM.WINDOWS)
@pytest.mark.parametrize("fs", LM.RATES)
def test_kernel_true_peak_against_f64_truth(monkeypatch, fs, ms):
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib())
    LM.check_kernel_true(eng, fs, ms)
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


def test_clicks(monkeypatch):
    _clean_env(monkeypatch)
    _, _, eng = E._engine(L.get_lib())
    T.clicks(eng)
    eng.close()


def test_speculative_form(monkeypatch):
    """With captured graphs: after pe_warmup every call replays the one graph with the launch count of the limiter-off
    setting, switching the limiter captures nothing once each has been seen, and a new window captures once."""
    _clean_env(monkeypatch)
    T.speculative(lambda: E._engine(L.get_lib()), graphs=True)


def test_off_is_the_parent(monkeypatch):
    _clean_env(monkeypatch)
    T.off_is_parent(lambda: E._engine(L.get_lib()))


def test_refusals(monkeypatch):
    from piper_amd.engine import Engine
    _clean_env(monkeypatch)
    cfg, _, eng = E._engine(L.get_lib())
    T.refusals(eng, cfg, lambda: Engine(onnx_path=os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx"), device=0))
    eng.close()


def test_group_voice_and_infer(monkeypatch, tmp_path):
    """EngineGroup.set_loudness(limiter=True) on devices [0, 0]: every member's call delivers under the ceiling and reports
    SHAPED, bit-equal floats and a level nearer the target than the same group without the limiter.
    PiperVoice.load(..., limiter=True) sets the engine, and what it delivers obeys the ceiling. piper_amd.infer --limiter
    writes WAVs that do."""
    from piper_amd.group import EngineGroup
    from piper_amd.voice import PiperVoice
    _clean_env(monkeypatch)
    cfg, w, _eng = E._engine(L.get_lib())
    _eng.close()
    fs = cfg.sample_rate
    ids = [W.synthetic_phoneme_ids(n, 300 + i, id_max=cfg.n_vocab - 1) for i, n in enumerate((19, 27, 22, 33))]
    zero = (0.0, 2.0, 0.0)
    got = {}
    for lim in (False, True):
        grp = EngineGroup(W.pack_blob(cfg, w), [0, 0])
        members = [grp.engine(i) for i in range(len(grp))]
        grp.set_loudness(-8.0, -1.0, limiter=lim, limiter_ms=5.0)
        assert all(m.loudness() == (-8.0, -1.0) and m.loudness_limiter() == (lim, 5.0, LM.window(fs, 5.0)[0]) for m in members)
        grp.set_seed(11)
        r = grp.synthesize_batch(ids, zero)
        who = grp.assignment(4)
        got[lim] = []
        for i, m in enumerate(members):
            mine = [u for u in range(4) if who[u] == i]
            if not mine:
                continue
            res = m.fetch(True, True)
            got[lim].append(res)
            if lim:
                flags = LM.check_delivery(m, res, got[False][len(got[True]) - 1], fs, -8.0, -1.0, 5.0, f"group engine {i}: ")
                assert any(f & LM.SHAPED for f in flags), flags
            for u in mine:
                assert any(p.size == r.pcm[u].size and np.array_equal(p, r.pcm[u]) for p in res.pcm), u
        for m in members:
            m.close()
        grp.close()

    model = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
    voice = PiperVoice.load(model, target_lufs=-8.0, peak_ceiling_db=-3.0, limiter=True, limiter_ms=4.0)
    rate = voice.config.sample_rate
    assert voice.session.loudness() == (-8.0, -3.0)
    assert voice.session.loudness_limiter() == (True, 4.0, LM.window(rate, 4.0)[0])
    raw = voice.synthesize_ids_to_raw([int(v) for v in W.synthetic_phoneme_ids(30, 3, id_max=39)], noise_scale=0.0,
                                      noise_w=0.0, length_scale=2.0)
    pcm = np.frombuffer(raw, np.int16)
    red, cnt, trim = voice.session.last_limiter()
    _, scale, peak, flags = voice.session.last_loudness()
    C = float(LM.ceiling_f32(-3.0))
    print(f"PiperVoice: max reduction {float(red[0]):.6f}, shaped samples {int(cnt[0])}, scale {float(scale[0]):.3f}, flags "
          f"{int(flags[0])}, max |pcm| {int(np.max(np.abs(pcm.astype(np.int32))))} (ceiling {32767.0 * C:.1f})")
    assert red.size == 1 and pcm.size > 0 and flags[0] & LC.LIMITED and flags[0] & LM.SHAPED and cnt[0] > 0 and red[0] > 0
    assert int(np.max(np.abs(pcm.astype(np.int32)))) <= 32767.0 * C
    assert float(scale[0]) * float(peak[0]) > 32767.0 * C          # the gain of the target, not the ceiling's
    voice.session.close()
    T.infer_limiter(L.get_lib(), tmp_path)
