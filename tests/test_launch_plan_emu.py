"""The level-2 profile rows Engine::conv assembles from a ConvPlan are the instantiations the launchers in kernels/ run for
that plan. The emulator records every launch as the launch macro names it (EMU_PLAN_TRACE, tests/emu/plan_trace.h); the rows
and the trace of the same plan-only calls are held against each other. No GPU."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so")
# the kernels Engine::conv and the grouped launchers go to
CONV_FAMILY = ("conv_mfma_kernel", "conv_mfma_group_kernel", "conv_split_kernel", "conv1x1_kernel", "conv_splitk_kernel",
               "conv_splitk16_kernel", "conv_splitk_group_kernel", "conv_splitk_sum_kernel", "gate4_kernel")
LDS_MAX = 160 * 1024

CODE = r'''
import json, os, sys
sys.path.insert(0, %r)
from piper_amd import _lib as L, weights as W
from piper_amd.engine import Engine
lib = L.bind(%r)
preset, B = sys.argv[1], int(sys.argv[2])
cfg = W.preset(preset)
eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), lib=lib)
eng.profile_enable(2)
eng.upload([W.synthetic_phoneme_ids(128, i, id_max=129) for i in range(B)], (0.667, 1.0, 0.8))
eng.run()
print(json.dumps([[r["name"], r["launches"]] for r in eng.profile()[5:] if r["launches"]]))
eng.close()
'''


def _strip(name):
    return re.sub(r"[ ()]", "", name).rstrip(">")


def _family(name):
    return name.split("<")[0] in CONV_FAMILY


def _plan(tmp_path, preset, B):
    trace = tmp_path / f"{preset}_{B}.trace"
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIPER_HIP_")}
    env.update(EMU_PLAN_ONLY="1", EMU_PLAN_FRAMES="417", EMU_PLAN_TRACE=str(trace))
    if not os.path.exists(EMU):
        subprocess.check_call(["make", "-C", ROOT, "emu"])
    res = subprocess.run([sys.executable, "-c", CODE % (ROOT, EMU), preset, str(B)], env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr
    rows = json.loads(res.stdout.strip().splitlines()[-1])
    launches = []
    for line in trace.read_text().splitlines():
        m = re.fullmatch(r"(.*) grid=(\d+),(\d+),(\d+) block=(\d+),(\d+),(\d+) lds=(\d+)", line)
        assert m, line
        launches.append((_strip(m.group(1)), tuple(int(v) for v in m.group(2, 3, 4)), int(m.group(8))))
    return rows, launches


def test_profile_rows_name_the_traced_instantiations(tmp_path):
    for preset, B in (("medium", 1), ("medium", 64), ("high", 1)):
        rows, launches = _plan(tmp_path, preset, B)
        assert launches, (preset, B)
        for name, grid, lds in launches:
            assert min(grid) > 0 and lds <= LDS_MAX, (preset, B, name, grid, lds)
        traced = [n for n, _, _ in launches if _family(n)]
        insts = sorted(set(traced))
        conv_rows = [(_strip(name.split("|")[0]), n) for name, n in rows if _family(name)]
        assert conv_rows and insts, (preset, B)
        for name, _ in conv_rows:
            assert len([i for i in insts if name.startswith(i)]) == 1, (preset, B, name, insts)
        for i in insts:
            assert len([name for name, _ in conv_rows if name.startswith(i)]) == 1, (preset, B, i, conv_rows)
        assert sum(n for _, n in conv_rows) == len(traced), (preset, B)
