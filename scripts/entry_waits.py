#!/usr/bin/env python3
"""Kernel entry sequences of a launch unit, read from its gfx950 assembly (no GPU needed).

For every kernel of the unit: the kernarg-preload length of its kernel descriptor (dwords that arrive in SGPRs at wave
launch) and the number of scalar waits (s_waitcnt with an lgkmcnt term) in front of the first vector-memory instruction.
Every such wait is one scalar-memory round trip on the launch's critical path. A wave-uniform lookup done on the vector side (one
load, waited for alone and read back with v_readfirstlane) counts as such a wait too. The unit is compiled with the command
`make` would use for its object (asked from make itself), with -S in place of -c and the device side only.

Usage: scripts/entry_waits.py [--json] piper_amd/csrc/kernels/launch_front.cpp [more units]
"""
import json
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "piper_amd/csrc/"
VMEM = re.compile(r"^(buffer_|global_|flat_|scratch_|tbuffer_)")


def find_tool(name):
    for d in (os.environ.get("ROCM", "/opt/rocm") + "/lib/llvm/bin", os.environ.get("ROCM", "/opt/rocm") + "/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def compile_command(unit):
    """The hipcc command line of the unit's object in the library build, as make prints it."""
    rel = os.path.relpath(os.path.abspath(unit), ROOT)
    if not rel.startswith(CSRC) or not rel.endswith(".cpp"):
        raise SystemExit(f"{unit}: not a translation unit under {CSRC}")
    obj = "build/gfx950/" + rel[len(CSRC):-4] + ".o"
    out = subprocess.check_output(["make", "-C", ROOT, "-s", "-n", "-B", obj], text=True)
    for line in out.splitlines():
        words = shlex.split(line)
        if "-c" in words and any(w.startswith("--offload-arch") for w in words):
            return words
    raise SystemExit(f"no compile command for {obj} in make's output")


def assembly(unit):
    words = compile_command(unit)
    with tempfile.TemporaryDirectory() as tmp:
        s = os.path.join(tmp, "unit.s")
        cmd = []
        skip = False
        for w in words:
            if skip:
                skip = False
            elif w == "-o":
                skip = True
            elif w == "-c":
                cmd += ["-S", "--cuda-device-only"]
            else:
                cmd.append(w)
        subprocess.check_call(cmd + ["-o", s], cwd=ROOT)
        with open(s) as f:
            return f.read()


def demangle(names):
    tool = find_tool("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.check_output([tool] + list(names), text=True).splitlines()
    res = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        d = re.sub(r"\(.*\)$", "", d)            # the parameter list
        res[n] = d.replace("pe::", "").replace(", ", ",")
    return res


def measure(unit):
    """{kernel name: (preload length in dwords, scalar waits before the first vector-memory instruction)}"""
    text = assembly(unit)
    preload = {}
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        pl = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", m.group(2))
        preload[m.group(1)] = int(pl.group(1)) if pl else 0
    lines = text.splitlines()
    waits = {}
    for name in preload:
        i = next((k + 1 for k, ln in enumerate(lines) if ln.startswith(name + ":")), None)
        if i is None:
            continue
        body = []
        while i < len(lines) and not lines[i].lstrip().startswith((".Lfunc_end", ".section", ".amdhsa_kernel")):
            body.append(lines[i].split(";")[0].strip())
            i += 1
        # A kernel with preloaded arguments starts with a prologue for firmware without the feature (it loads them and
        # branches over the padding to the entry the descriptor names, 256 bytes in); where preloading works it never runs.
        if preload[name] > 0:
            for j, ins in enumerate(body[:64]):
                if ins.startswith(".p2align") and any(x.startswith("s_branch") for x in body[:j]):
                    body = body[j + 1:]
                    break
        # A wave-uniform lookup done on the vector side -- one load, waited for (vmcnt(0)) before any other vector-memory
        # instruction and read back with v_readfirstlane -- is no operand load: it is a round trip like a scalar wait,
        # counted as one, and the count goes on behind it.
        n = 0
        k = 0
        while k < len(body):
            ins = body[k]
            if VMEM.match(ins):
                j = next((q for q in range(k + 1, len(body))
                          if VMEM.match(body[q]) or (body[q].startswith("s_waitcnt") and "vmcnt(0)" in body[q])), None)
                dest = re.match(r"\S+\s+(v\d+)\b", ins)
                uniform = (j is not None and body[j].startswith("s_waitcnt") and dest is not None and
                           any(re.match(r"v_readfirstlane_b32 s\d+, %s$" % dest.group(1), x) for x in body[j + 1:j + 16]))
                if not uniform:
                    break
                n += 1
                k = j
            elif ins.startswith("s_waitcnt") and "lgkmcnt" in ins:
                n += 1
            k += 1
        waits[name] = n
    names = demangle(sorted(waits))
    return {names[k]: (preload[k], waits[k]) for k in waits}


def main(argv):
    as_json = "--json" in argv
    units = [a for a in argv if not a.startswith("--")]
    if not units:
        raise SystemExit(__doc__)
    res = {}
    for u in units:
        res[os.path.basename(u)] = measure(u)
    if as_json:
        print(json.dumps(res, indent=1, sort_keys=True))
        return
    for u, ks in res.items():
        print(f"### {u}\n")
        print("| kernel | preload dwords | scalar waits before first vector load |")
        print("|---|---|---|")
        for k in sorted(ks):
            print(f"| `{k}` | {ks[k][0]} | {ks[k][1]} |")
        print()


if __name__ == "__main__":
    main(sys.argv[1:])
