"""SynthesisConfig::truePeak of include/piper.hpp (tests/cpp/test_true_peak.cpp): the field reaches the engine as the kind
of ceiling, with and without targetLufs, and comes back out. The program runs against the emulator build here and against
the shipped library on the GPU (-m gpu)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")


def run(binary, lib, targets):
    exe = os.path.join(ROOT, "tests", "cpp", binary)
    deps = [os.path.join(ROOT, lib), os.path.join(ROOT, "tests", "cpp", "test_true_peak.cpp"),
            os.path.join(ROOT, "include", "piper.hpp"), os.path.join(ROOT, "include", "piper_hip.h")]
    # (a program that is newer than the library and the sources it was built from is used as it is)
    if not all(os.path.exists(f) for f in [exe] + deps) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["make", "-C", ROOT] + targets, stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, MODEL], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"phrase (\d+) t=(\S+) p=(\S+) scale=(\S+) flags=(\d+)", out.stdout)
    m = re.search(r"^OK phrases=2 oversample=(\d+) half_width=(\d+) ceiling=(\S+)", out.stdout, re.M)
    assert len(rows) == 2 and m
    assert (int(m.group(1)), int(m.group(2))) == (12, 18)          # the voice's 16000 Hz
    C = float(m.group(3))
    for _, t, p, scale, flags in rows:
        t, p, scale, flags = float(t), float(p), float(scale), int(flags)
        assert t > 0 and p > 0 and flags & 4, (t, p, flags)          # T = -5 LUFS: the ceiling wins
        assert scale * max(t, p) <= 32767.0 * C * (1 + 1e-6)


def test_true_peak_through_piper_hpp_on_emulator():
    run("test_true_peak_emu", os.path.join("tests", "emu", "libpiper_hip_emu.so"), ["emu", "tests/cpp/test_true_peak_emu"])


@pytest.mark.gpu
def test_true_peak_through_piper_hpp():
    run("test_true_peak", os.path.join("piper_amd", "libpiper_hip.so"), ["tests/cpp/test_true_peak"])
