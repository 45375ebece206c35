"""SynthesisConfig::limiter / limiterMs of include/piper.hpp (tests/cpp/test_limiter.cpp): the fields reach the engine as the
look-ahead limiter's setting, with and without targetLufs, and come back out; textToAudio delivers under the ceiling and
reports SHAPED. The program runs against the emulator build here and against the shipped library on the GPU (-m gpu)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")


def run(binary, lib, targets):
    exe = os.path.join(ROOT, "tests", "cpp", binary)
    deps = [os.path.join(ROOT, lib), os.path.join(ROOT, "tests", "cpp", "test_limiter.cpp"),
            os.path.join(ROOT, "include", "piper.hpp"), os.path.join(ROOT, "include", "piper_hip.h")]
    # (a program that is newer than the library and the sources it was built from is used as it is)
    if not all(os.path.exists(f) for f in [exe] + deps) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["make", "-C", ROOT] + targets, stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, MODEL], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"phrase (\d+) red=(\S+) shaped=(\d+) trim=(\S+) scale=(\S+) flags=(\d+)", out.stdout)
    m = re.search(r"^OK phrases=2 window=(\d+) max=(\d+) differs=(\d) ceiling=(\S+)", out.stdout, re.M)
    assert len(rows) == 2 and m
    assert int(m.group(1)) == 64                                     # 4 ms at the voice's 16000 Hz
    C = float(m.group(4))
    assert int(m.group(2)) <= 32767.0 * C and int(m.group(3)) == 1
    shaped = 0
    for _, red, cnt, trim, scale, flags in rows:
        red, cnt, trim, flags = float(red), int(cnt), float(trim), int(flags)
        assert trim == 1.0 and bool(flags & 8) == (cnt > 0) == (red > 0), (red, cnt, flags)
        assert not flags & 8 or flags & 4                            # SHAPED rows are LIMITED rows
        shaped += bool(flags & 8)
    assert shaped >= 1                                               # T = -8 LUFS under -2 dB: the ceiling conflicts


def test_limiter_through_piper_hpp_on_emulator():
    run("test_limiter_emu", os.path.join("tests", "emu", "libpiper_hip_emu.so"), ["emu", "tests/cpp/test_limiter_emu"])


@pytest.mark.gpu
def test_limiter_through_piper_hpp():
    run("test_limiter", os.path.join("piper_amd", "libpiper_hip.so"), ["tests/cpp/test_limiter"])
