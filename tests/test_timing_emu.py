"""Timing plans (pe_timing: per-id rates, forced durations, a target frame count) on the test-only emulator build of the
engine (tests/emu). The cases and their checks live in tests/timing_case.py; the GPU counterpart is tests/test_gpu_timing.py
(-m gpu). Float gate against the timed oracle: 1e-4."""
import json
import os
import subprocess
import sys

import pytest

from piper_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import timing_case as TC                                 # noqa: E402

GATE = 1e-4


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


@pytest.fixture
def voice(emu_lib, monkeypatch, request):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    v = TC.Voice(getattr(request, "param", "tiny"), lib=emu_lib)
    yield v
    v.close()


both = pytest.mark.parametrize("voice", ["tiny", "tiny-ms"], indirect=True)


def test_plan_kernel_equals_the_restatement(voice):
    """Case 1: pe_debug_timing for T from 1 to 8192, every mode, ties, both clamps, the smallest and the largest target."""
    TC.check_kernel_alone(voice.eng)
    TC.check_w_against_float32(voice.eng)


@both
def test_a_plan_that_says_nothing_changes_nothing(voice):
    TC.check_silent_plan(voice)


@both
def test_durations_fed_back_give_the_same_audio(voice):
    """Case 3: whatever duration noise is passed, with fewer launches than a call with one id left free; on the
    multi-speaker voice also with other speakers."""
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
    """Case 7: the timed lock-step stream against the timed call, a timed newcomer in a pool of untimed residents."""
    TC.check_streams(voice)


@both
def test_refused_plans_leave_a_live_stream_alone(voice):
    TC.check_errors(voice)


@both
def test_untimed_calls_are_what_they_were(voice):
    TC.check_untimed_untouched(voice)


def test_round_trip_and_target_on_the_192_channel_small_call_path(emu_lib, monkeypatch):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", "1")
    TC.check_192_channels(emu_lib)


def test_piper_voice_and_jsonl_driver_take_timing(emu_lib, tmp_path):
    TC.check_voice_and_driver(emu_lib, tmp_path)


def test_timed_batch_does_not_depend_on_wave_order():
    """Case 4 once per fiber order of the emulator (ascending, EMU_ORDER=reverse, =shuffle), each in a process of its own:
    identical durations and int16 output -- the plan kernel's reductions, its bitwise search and its scan do not depend on
    the order in which waves reach a barrier."""
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    outs = []
    for order in ("", "reverse", "shuffle"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "emu", "timing_order_case.py")], capture_output=True,
                           text=True, timeout=900, env=dict(os.environ, EMU_ORDER=order))
        assert p.returncode == 0, p.stderr[-2000:]
        outs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert outs[0]["durations"] == outs[1]["durations"] == outs[2]["durations"], outs
    assert outs[0]["frames"] == outs[1]["frames"] == outs[2]["frames"]
    assert outs[0]["pcm_sha256"] == outs[1]["pcm_sha256"] == outs[2]["pcm_sha256"], outs
