"""G.711 delivery on the MI355X (run with -m gpu): the cases of tests/test_g711_emu.py on the device -- the law on the host,
the kernel alone on both laws and both forms, whole utterances on every route of the delivery stage at every rate on poisoned
workspaces (also under PIPER_HIP_MATRIX=f16x3), the speculative one-graph form with captured graphs, the untouched s16 path,
batch stream and pool under every stream setting at the native rate and at 8000 Hz, the one-utterance stream and the
refusals. Every comparison is bit-exact."""
import json
import os
import sys

import pytest

from piper_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import g711_case as G                                    # noqa: E402
import stream_batch_case as K                            # noqa: E402
import stream_pool_case as P                             # noqa: E402
import test_g711_emu as T                                # noqa: E402

pytestmark = pytest.mark.gpu


def _clean_env(monkeypatch, env=None):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))


def test_law(monkeypatch):
    _clean_env(monkeypatch)
    G.check_law(L.get_lib())


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_kernel_rows(monkeypatch, fmt):
    _clean_env(monkeypatch)
    _, _, eng = T._engine(L.get_lib())
    G.check_kernel_rows(eng, fmt)
    eng.close()


@pytest.mark.parametrize("fmt", G.FORMATS)
def test_kernel_flat(monkeypatch, fmt):
    _clean_env(monkeypatch)
    _, _, eng = T._engine(L.get_lib())
    G.check_kernel_flat(eng, fmt)
    eng.close()


@pytest.mark.parametrize("rate", [0, 8000, 48000])
def test_whole_utterances(monkeypatch, rate):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = T._engine(L.get_lib())
    G.whole_utterances(eng, cfg, rate, K, T.STRETCH)
    eng.close()


def test_whole_utterances_f16x3(monkeypatch):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1, "PIPER_HIP_MATRIX": "f16x3"})
    cfg, _, eng = T._engine(L.get_lib())
    G.whole_utterances(eng, cfg, 0, K, T.STRETCH)
    eng.close()


def test_speculative_form(monkeypatch):
    """With captured graphs: after pe_warmup every call replays the one graph, a law costs exactly one launch more, and once
    each format has been seen, alternating s16 / ulaw / alaw captures nothing."""
    _clean_env(monkeypatch)
    G.speculative(lambda: T._engine(L.get_lib()), graphs=True)


def test_off_is_the_parent(monkeypatch):
    _clean_env(monkeypatch)
    G.off_is_parent(lambda: T._engine(L.get_lib()), K)


@pytest.mark.parametrize("rate", [None, 8000])
def test_streams(monkeypatch, rate):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = T._engine(L.get_lib())
    G.check_streams(eng, cfg, K, P, rate)
    eng.close()


def test_pool_multi_speaker(monkeypatch):
    """The pool on the multi-speaker voice (its conditioning rows live with the slots) under every stream setting."""
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = T._engine(L.get_lib(), "tiny-ms")
    G.check_streams(eng, cfg, K, P, None, [c for c in G.STREAM_CASES if c[1] == "pool"], multi_speaker=True)
    eng.close()


@pytest.mark.parametrize("rate", [None, 8000])
def test_one_utterance_stream(monkeypatch, rate):
    _clean_env(monkeypatch, {"PIPER_HIP_DEBUG_POISON": 1})
    cfg, _, eng = T._engine(L.get_lib())
    G.check_one_stream(eng, cfg, K, rate)
    eng.close()


def test_refusals(monkeypatch):
    _clean_env(monkeypatch)
    cfg, _, eng = T._engine(L.get_lib())
    G.check_refusals(eng, cfg, K, P)
    eng.close()


def test_piper_voice_and_infer(monkeypatch, tmp_path):
    """PiperVoice.load(..., sample_format=) sets the engine; the voice's bytes, silence and WAV, and the command-line tool."""
    from piper_amd.voice import PiperVoice
    _clean_env(monkeypatch)
    voice = PiperVoice.load(T.MODEL, sample_format="alaw")
    assert voice.sample_format == "alaw" == voice.session.sample_format
    G.check_voice(voice, tmp_path)
    voice.session.close()
    plain = PiperVoice.load(T.MODEL)
    assert plain.sample_format == "s16" == plain.session.sample_format
    plain.session.close()
    G.check_infer(L.get_lib(), tmp_path, T.MODEL)
