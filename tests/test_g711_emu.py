"""G.711 delivery (pe_set_sample_format: one mu-law or A-law code per delivered int16 sample, companded by g711_kernel) on the
test-only emulator build of the engine: the law on the host, the kernel alone on the shapes of tests/g711_case.py, whole
utterances on every route of the delivery stage at the native rate and at 8000 / 48000 Hz on poisoned workspaces, the
speculative one-utterance form, the untouched s16 path, every kind of stream, the refusals and the fronts (PiperVoice, the
command-line tool). Every comparison is bit-exact. The GPU counterpart is tests/test_gpu_g711.py (-m gpu)."""
import os
import subprocess
import sys

import pytest

from piper_amd import _lib as L
from piper_amd import weights as W
from piper_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import g711_case as G                                    # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402

STRETCH = 60             # frames of the third utterance, as in tests/test_loudness_emu.py


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


def _engine(lib, preset="tiny", device=0):
    cfg = W.preset(preset)
    w = W.synthetic_weights(cfg, 1234)
    return cfg, w, Engine(blob=W.pack_blob(cfg, w), lib=lib, device=device)


def _poisoned(lib, preset="tiny"):
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("PIPER_HIP_DEBUG_POISON", "1")
        return _engine(lib, preset)


# ---- 1. the law, on the host
def test_law(emu_lib):
    G.check_law(emu_lib)


# ---- 2. the kernel alone
@pytest.mark.parametrize("fmt", G.FORMATS)
def test_kernel_rows(emu_lib, fmt):
    _, _, eng = _engine(emu_lib)
    G.check_kernel_rows(eng, fmt)
    eng.close()


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_kernel_flat(emu_lib, fmt):
    _, _, eng = _engine(emu_lib)
    G.check_kernel_flat(eng, fmt)
    eng.close()


# ---- 3. whole utterances
# (the emulator takes seconds per call: the native rate runs every route of the delivery stage, the converted rates two
# each, between them all four; the GPU twin runs every route at every rate)
@pytest.mark.parametrize("rate,settings", [(0, None), (8000, ("loudness", "limiter")), (48000, ("peak", "true-peak limiter"))])
def test_whole_utterances(emu_lib, monkeypatch, rate, settings):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    cfg, _, eng = _engine(emu_lib)
    G.whole_utterances(eng, cfg, rate, K, STRETCH, settings)
    eng.close()


def test_whole_utterances_f16x3(emu_lib, monkeypatch):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    monkeypatch.setenv("PIPER_HIP_MATRIX", "f16x3")
    cfg, _, eng = _engine(emu_lib)
    G.whole_utterances(eng, cfg, 0, K, STRETCH, ("limiter",))
    eng.close()


# ---- 4. the speculative one-utterance form
def test_speculative_form(emu_lib):
    G.speculative(lambda: _engine(emu_lib), graphs=False)


# ---- 5. off is the parent
def test_off_is_the_parent(emu_lib):
    G.off_is_parent(lambda: _engine(emu_lib), K)


# ---- 6. streams
# (a drain of a stream costs the emulator a quarter of a minute: a covering subset of tests/g711_case.py's STREAM_CASES --
# every setting, both kinds of stream, both rates, both laws; the GPU twin runs the whole cross product)
@pytest.mark.parametrize("rate,case,fmt", [(None, ("chunk", "batch"), "ulaw"), (None, ("limiter", "batch"), "alaw"),
                                           (None, ("running", "pool"), "alaw"), (8000, ("loudness", "batch"), "alaw"),
                                           (8000, ("limiter", "pool"), "ulaw")])
def test_streams(emu_lib, rate, case, fmt):
    cfg, _, eng = _poisoned(emu_lib)
    G.check_streams(eng, cfg, K, P, rate, (case,), (fmt,))
    eng.close()


@pytest.mark.parametrize("rate,settings", [(None, ("chunk", "limiter")), (8000, ("limiter",))])
def test_one_utterance_stream(emu_lib, rate, settings):
    cfg, _, eng = _poisoned(emu_lib)
    G.check_one_stream(eng, cfg, K, rate, settings)
    eng.close()


def test_refusals(emu_lib):
    cfg, _, eng = _engine(emu_lib)
    G.check_refusals(eng, cfg, K, P)
    eng.close()


# ---- 7. fronts
MODEL = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")


def test_piper_voice(emu_lib, tmp_path):
    import json
    from piper_amd.config import PiperConfig
    from piper_amd.voice import PiperVoice
    with open(MODEL + ".json", "r", encoding="utf-8") as f:
        config = PiperConfig.from_dict(json.load(f))
    voice = PiperVoice(config=config, session=Engine(onnx_path=MODEL, lib=emu_lib))
    G.check_voice(voice, tmp_path)
    voice.session.close()


def test_infer_sample_format(emu_lib, tmp_path):
    G.check_infer(emu_lib, tmp_path, MODEL)
