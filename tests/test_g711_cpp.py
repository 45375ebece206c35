"""SynthesisConfig::sampleFormat of include/piper.hpp (tests/cpp/test_g711.cpp): synthesizeEncoded and textToEncodedAudio
deliver g711 of what synthesize and textToAudio deliver, silences as the law's zero code; textToWavFile writes the G.711
header. The program checks itself bit for bit; it runs against the emulator build here and against the shipped library on
the GPU (-m gpu)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = os.path.join(ROOT, "tests", "golden", "tiny_voice.onnx")


def run(binary, lib, targets):
    exe = os.path.join(ROOT, "tests", "cpp", binary)
    deps = [os.path.join(ROOT, lib), os.path.join(ROOT, "tests", "cpp", "test_g711.cpp"),
            os.path.join(ROOT, "include", "piper.hpp"), os.path.join(ROOT, "include", "piper_hip.h")]
    # (a program that is newer than the library and the sources it was built from is used as it is)
    if not all(os.path.exists(f) for f in [exe] + deps) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in deps):
        subprocess.check_call(["make", "-C", ROOT] + targets, stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, MODEL], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stderr
    rows = re.findall(r"^law (\w+) tag=(\d+) samples=(\d+) one=(\d+) zero=0x(\w+) silence=(\d+)", out.stdout, re.M)
    assert [(r[0], int(r[1]), r[4]) for r in rows] == [("ulaw", 7, "FF"), ("alaw", 6, "D5")], rows
    assert rows[0][2] == rows[1][2] and int(rows[0][2]) > int(rows[0][3]) > 0 and int(rows[0][5]) == 160
    assert re.search(r"^OK$", out.stdout, re.M)


def test_g711_through_piper_hpp_on_emulator():
    run("test_g711_emu", os.path.join("tests", "emu", "libpiper_hip_emu.so"), ["emu", "tests/cpp/test_g711_emu"])


@pytest.mark.gpu
def test_g711_through_piper_hpp():
    run("test_g711", os.path.join("piper_amd", "libpiper_hip.so"), ["tests/cpp/test_g711"])
