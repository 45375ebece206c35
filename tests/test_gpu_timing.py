"""Timing plans on the MI355X (run with -m gpu): the cases of tests/test_timing_emu.py on the device, where stage A is a
captured graph -- and, on top, the replay of that graph under new plan values, a 4100-id utterance stretched to 6000 frames
and one targeted utterance of the full medium voice. Float gate against the timed oracle: the project's 2e-4."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

from piper_amd import _lib as L
from piper_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import timing_case as TC                                 # noqa: E402

pytestmark = pytest.mark.gpu
GATE = 2e-4


@pytest.fixture
def voice(monkeypatch, request):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    v = TC.Voice(getattr(request, "param", "tiny"), lib=L.get_lib())
    yield v
    v.close()


both = pytest.mark.parametrize("voice", ["tiny", "tiny-ms"], indirect=True)


def test_plan_kernel_equals_the_restatement(voice):
    TC.check_kernel_alone(voice.eng)
    TC.check_w_against_float32(voice.eng)


@both
def test_a_plan_that_says_nothing_changes_nothing(voice):
    TC.check_silent_plan(voice)


@both
def test_durations_fed_back_give_the_same_audio(voice):
    TC.check_round_trip(voice, GATE)


@both
def test_mixed_timed_batch_against_the_timed_oracle(voice):
    TC.check_mixed(voice, GATE)


@both
def test_every_utterance_of_a_timed_batch_is_what_it_is_alone(voice):
    TC.check_batch_independence(voice)


@both
def test_targets_are_exact_in_calls_streams_and_the_pool(voice):
    TC.check_targets_exact(voice)


@both
def test_timed_streams(voice):
    TC.check_streams(voice)


@both
def test_refused_plans_leave_a_live_stream_alone(voice):
    TC.check_errors(voice)


@both
def test_untimed_calls_are_what_they_were(voice):
    """Case 9 with captured graphs: the untimed one-utterance call before and after the burst is the speculative one-graph
    form, and the burst makes it capture nothing new."""
    caps = TC.check_untimed_untouched(voice)
    assert caps > 0 and voice.eng.speculation_stats[0] >= 2


def test_round_trip_and_target_on_the_192_channel_small_call_path(voice):
    TC.check_192_channels(L.get_lib())


def test_piper_voice_and_jsonl_driver_take_timing(voice, tmp_path):
    TC.check_voice_and_driver(L.get_lib(), tmp_path)


def test_stage_a_graph_replays_under_new_plan_values(voice):
    """(b) The same timed shapes twice with different rates, forced values and targets, the engine drawing its own noise (so
    that both halves are graphs): the second call captures nothing, and its durations obey ITS plan."""
    eng = voice.eng
    ids, sc, sids, nw, _ = voice.sub([0, 1, 2])
    rng = np.random.default_rng(3)
    # the workspaces sized beforehand, as a server does: a first call that grows stage B's drops every graph, stage A's of
    # that same call included, and the second call would capture it again whatever the plan
    eng.warmup(max_batch=3, max_ids=32, frames_per_id=8.0)
    assert eng.graph_stats == (0, 0)

    def plan(k):
        rate = [rng.uniform(0.5, 2.0, len(s)).astype(np.float32) for s in ids]
        forced = [np.full(len(s), -1, np.int32) for s in ids]
        forced[1][4 + k], forced[2][1] = 3 + 5 * k, k
        return rate, forced, [30 + k, 60 + 3 * k, 70 - 2 * k]      # (every call's longest utterance in one frame bucket)

    caps = None
    for k in range(3):
        rate, forced, target = plan(k)
        r = eng.synthesize_batch(ids, sc, sids=sids, noise_w=nw, timing=TC.Timing(rate=rate, durations=forced, target_frames=target))
        d = TC.split(eng.durations(), ids)
        for b in range(3):
            want, fr = TC.restate(eng.debug_tensor("plan_w", b)[0], forced[b], target[b])
            assert np.array_equal(d[b], want) and int(r.frames[b]) == fr, (k, b)
        assert list(r.frames) == target
        if k == 0:
            caps = eng.graph_stats[1]                    # (stage A under a plan, stage B)
            assert eng.graph_stats == (2, 2), eng.graph_stats
        else:
            assert eng.graph_stats == (2, caps), (k, caps, eng.graph_stats)
    assert caps == 2


def test_long_utterance_stretched_to_a_target(voice):
    """(c) 4100 ids on the tiny voice with a target of 6000 frames: 17 ids per thread in the plan kernel, the regulator's
    search in global memory."""
    eng = voice.eng
    ids = [W.synthetic_phoneme_ids(4100, 11, id_max=voice.cfg.n_vocab - 1)]
    r = eng.synthesize_batch(ids, (0.667, 1.0, 0.8), timing=TC.Timing(target_frames=[6000]))
    assert r.frames[0] == 6000 and r.pcm[0].size == 6000 * eng.hop
    d = eng.durations()
    want, fr = TC.restate(eng.debug_tensor("plan_w", 0)[0], np.full(4100, -1), 6000)
    assert fr == 6000 and np.array_equal(d, want) and d.min() >= 1
    assert np.isfinite(r.audio[0]).all()


def test_full_medium_voice_with_a_target(monkeypatch, tmp_path):
    """(d) One 40-id utterance of the full-size medium voice under a target 25 % above its natural length: the frame count
    exact, the durations those of the restatement, the audio that of the timed oracle."""
    from oracle import vits_oracle as O
    from oracle import voice_skeleton as S
    from piper_amd.engine import Engine
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    path = S.fill("medium_voice.onnx", str(tmp_path))
    lib = L.get_lib()
    blob, n = C.c_void_p(), C.c_size_t()
    assert lib.pe_onnx_to_blob(path.encode(), C.byref(blob), C.byref(n)) == 0, lib.pe_last_error()
    data = C.string_at(blob, n.value)
    lib.pe_free(blob)
    cfg, w = W.unpack_blob(data)
    eng = Engine(onnx_path=path, device=0)
    T = 40
    ids = W.synthetic_phoneme_ids(T, 7, id_max=min(eng.num_symbols - 1, 129))
    rng = np.random.default_rng(40)
    nw = rng.standard_normal((1, 2, T)).astype(np.float32)
    nz = rng.standard_normal((1, 192, 12 * T + 64)).astype(np.float32)
    sc = (0.667, 1.0, 0.8)
    nat = int(eng.synthesize_batch([ids], sc, noise_w=nw, noise_z=nz).frames[0])
    target = int(round(1.25 * nat))
    assert target <= nz.shape[-1]
    r = eng.synthesize_batch([ids], sc, noise_w=nw, noise_z=nz, timing=TC.Timing(target_frames=[target]))
    d = eng.durations()
    want, fr = TC.restate(eng.debug_tensor("plan_w", 0)[0], np.full(T, -1), target)
    assert r.frames[0] == target == fr and np.array_equal(d, want)
    ra, rp = TC.timed_oracle(O.to_torch(w), cfg, ids, d, nz[0], sc[0])
    TC.assert_audio(r.audio[0], r.pcm[0], ra, rp, GATE, "medium voice under a target")
    eng.close()
