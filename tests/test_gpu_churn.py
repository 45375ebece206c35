"""Settings churn does not leak into results, on the MI355X (run with -m gpu): the case of tests/churn_case.py with the policy's
debug-poison knob on and off, with captured graphs."""
import json
import os
import sys

import pytest

from piper_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import churn_case as CH                                  # noqa: E402
import test_loudness_emu as E                            # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("poison", [1, 0])
def test_settings_churn_does_not_leak_into_results(monkeypatch, poison):
    for k in [x["env"] for x in json.loads(L.get_lib().pe_policy_describe().decode())] + ["PIPER_HIP_MATRIX"]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("PIPER_HIP_DEBUG_POISON", str(poison))
    CH.check(lambda: E._engine(L.get_lib()))
