"""The mixed timed batch of tests/timing_case.py (case 4) once on the emulator build under the fiber order EMU_ORDER names
(the emulator reads the variable once per process): prints one JSON line with the durations, the frame counts and a digest
of the int16 output. Child process of tests/test_timing_emu.py."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import timing_case as TC                                 # noqa: E402


def main():
    os.environ["PIPER_HIP_DEBUG_POISON"] = "1"
    v = TC.Voice("tiny", lib=TC.L.bind(os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")))
    out = TC.mixed_digest(v)
    v.close()
    print(json.dumps(dict(out, order=os.environ.get("EMU_ORDER", ""))))


if __name__ == "__main__":
    main()
