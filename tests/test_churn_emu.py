"""Settings churn does not leak into results, on the test-only emulator build of the engine: the case of tests/churn_case.py
with the policy's debug-poison knob on and off. The GPU counterpart is tests/test_gpu_churn.py (-m gpu)."""
import os
import subprocess
import sys

import pytest

from piper_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import churn_case as CH                                  # noqa: E402
import test_loudness_emu as E                            # noqa: E402


@pytest.fixture(scope="module")
def emu_lib():
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    return L.bind(EMU)


@pytest.mark.parametrize("poison", [1, 0])
def test_settings_churn_does_not_leak_into_results(emu_lib, monkeypatch, poison):
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", str(poison))
    CH.check(lambda: E._engine(emu_lib))
