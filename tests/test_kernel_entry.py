"""Entry sequences of the one-utterance text-encoder / flow kernels, read from the gfx950 assembly of their launch unit
(scripts/entry_waits.py; needs the compiler, no GPU): their leading arguments are preloaded into SGPRs and at most one
scalar-memory wait stands in front of the first vector load."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
KERNELS = ["dds_layer4_kernel", "colchain4_kernel<false>", "colchain4_kernel<true>", "lngemm4_kernel",
           "attn4_kernel<96,false>", "ffn_kernel"]


@pytest.fixture(scope="module")
def front():
    if not (os.path.exists(HIPCC) or shutil.which("hipcc")):
        pytest.skip("hipcc is not installed")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import entry_waits
    finally:
        sys.path.pop(0)
    return entry_waits.measure(os.path.join(ROOT, "piper_amd", "csrc", "kernels", "launch_front.cpp"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_entry_is_preloaded_and_waits_at_most_once(front, kernel):
    assert kernel in front, sorted(front)
    preload, waits = front[kernel]
    print(kernel, "preload dwords", preload, "scalar waits before the first vector load", waits)
    assert preload > 0
    assert waits <= 1
