"""SynthesisConfig::targetLufs / peakCeilingDb of include/piper.hpp (tests/cpp/test_loudness.cpp): textToAudio batches the
phrases of a sentence, so with a target every phrase lands on the same level. The program runs against the emulator build
here and against the shipped library on the GPU (-m gpu)."""
import math
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")
SHORT, UNMEASURABLE, LIMITED = 1, 2, 4


def run(binary, lib, targets):
    exe = os.path.join(ROOT, "tests", "cpp", binary)
    deps = [os.path.join(ROOT, lib), os.path.join(ROOT, "tests", "cpp", "test_loudness.cpp"),
            os.path.join(ROOT, "include", "piper.hpp"), os.path.join(ROOT, "include", "piper_hip.h")]
    # (a program that is newer than the library and the sources it was built from is used as it is)
    if not all(os.path.exists(f) for f in [exe] + deps) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["make", "-C", ROOT] + targets, stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, MODEL], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"phrase (\d+) L=(\S+) scale=(\S+) peak=(\S+) flags=(\d+)", out.stdout)
    assert len(rows) == 2 and re.search(r"^OK phrases=2 at_target=\d+ samples=\d+", out.stdout, re.M)
    delivered = []
    for _, L, scale, peak, flags in rows:
        L, scale, peak, flags = float(L), float(scale), float(peak), int(flags)
        assert not flags & UNMEASURABLE and peak > 0
        assert peak * scale <= 32767.0 * 10.0 ** (-1.5 / 20.0) * (1 + 1e-6)
        if not flags & (SHORT | LIMITED):
            delivered.append(L + 20.0 * math.log10(scale / 32767.0))
    # both phrases are long enough for gated blocks and quiet enough for the ceiling: both sit on the target
    assert len(delivered) == 2 and all(abs(d + 24.0) <= 1e-3 for d in delivered), (rows, delivered)


def test_target_lufs_through_piper_hpp_on_emulator():
    run("test_loudness_emu", os.path.join("tests", "emu", "libpiper_hip_emu.so"), ["emu", "tests/cpp/test_loudness_emu"])


@pytest.mark.gpu
def test_target_lufs_through_piper_hpp():
    run("test_loudness", os.path.join("piper_amd", "libpiper_hip.so"), ["tests/cpp/test_loudness"])
