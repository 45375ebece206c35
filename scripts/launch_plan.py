"""Launch plan of the engine on the kernel emulator, no GPU needed: what a refactor of the launch code must leave unchanged.

    make emu && python scripts/launch_plan.py OUT [--root CHECKOUT] [--jobs 16] [--env KNOB=VALUE]

runs a fixed list of cases, each in a fresh process (policy knobs, the matrix mode and the emulator's plan-only mode are
read once per process), and writes per case under OUT/<case>/

    trace.txt     one line per kernel launch (tests/emu/plan_trace.h, EMU_PLAN_TRACE): instantiation, grid, block, LDS bytes
    rows.json     the level-2 profile rows: name, launches, flops, bytes
    launches.txt  run_launches after each call
    audio.f32, pcm.i16, durations.i32   (executing cases only) what the calls delivered

Plan-only cases (EMU_PLAN_ONLY=1, EMU_PLAN_FRAMES set) take the full-size voices: presets medium and high, batch 1..64,
16..500 ids, 60..1200 frames per utterance, the four matrix modes, every routing knob changed one at a time, and one
chunk of each stream kind. Executing cases run the tiny voices through the same knobs and stream kinds; two of them have
the 192 channels of the full-size voices (the coupling flow's 4-column route: Engine::plan_flow) and also run at forced
frame counts that are no multiples of 4, under every setting of the flow's own knobs. Every case makes two consecutive calls. Run it on two checkouts (--root: the tree whose package and emulator library are used) and
`diff -r` the two output trees; the last line printed is a JSON summary with a sha256 over the tree
(profiles/launch_plan.md)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = (("SPLITK_MAX", 0), ("SPLITK16", 0), ("SPLITK16", 3), ("WIDE_SPLITK", 0), ("WIDE_SPLITK", 2), ("GATE4", 0),
         ("GATE4", 2), ("GATE_HALF", 0), ("CONV1X1", 0), ("GROUP_MRF", 0), ("GROUP_MRF", 2), ("GROUP_TILED", 0),
         ("GROUP_MAXB", 0), ("MRF", 0), ("MRF", 2), ("MRF_TAIL", 0), ("TPB", 3), ("PROF_SITES", 1),
         # the coupling flow's route (Engine::plan_flow)
         ("COLCHAIN", 0), ("COLCHAIN", 2), ("COL4", 0), ("COL4", 2), ("CHAIN_RS", 0), ("STACK_PRE", 0),
         ("WN_COMPOSE", 0), ("WN_COMPOSE", 2), ("WN_COMPOSE", 3), ("WN_COMPOSE", 4))
KNOB_PAIRS = ((("WN_COMPOSE", 1), ("CHAIN_RS", 0)), (("WN_COMPOSE", 4), ("GATE4", 0)))
# tiny with the 192 channels of medium / high (tests/one_utterance_truth_case.py: tiny192; tests/test_wn_compose_emu.py: its
# multi-speaker variant): the executing voices on which the 4-column flow route runs
WIDE = {"tiny192": dict(hidden=192, inter=192, filter=96, n_layers=2)}
WIDE["tiny192-ms"] = dict(WIDE["tiny192"], n_speakers=4, gin=16)
# forced frame counts that are no multiples of 4 (ragged 4-column tiles): one utterance, and two
FORCED = ((13,), (3, 13))
MATRIX = ("f32", "bf16x3", "f16x3", "bf16x6")
STREAMS = ("stream", "stream_batch", "pool")
SCALES = (0.667, 1.0, 0.8)


def cases():
    out = []

    def add(name, preset, **kw):
        c = dict(name=name, preset=preset, B=1, ids=128, frames=None, matrix="f32", env={}, kind="call", forced=None)
        c.update(kw)
        out.append(c)

    knobs = [(kv,) for kv in KNOBS] + list(KNOB_PAIRS)
    tag = lambda kvs: "_".join(f"{k}{v}" for k, v in kvs)
    env = lambda kvs: {"PIPER_HIP_" + k: str(v) for k, v in kvs}

    for preset in ("medium", "high"):
        for B in (1, 2, 4, 16, 64):
            for ids in (16, 64, 128, 500):
                add(f"plan/{preset}/b{B}_i{ids}", preset, B=B, ids=ids, frames=417)
        for frames in (60, 1200):
            for B in (1, 4, 16):
                add(f"plan/{preset}/b{B}_f{frames}", preset, B=B, frames=frames)
        for m in MATRIX[1:]:
            for B, frames in ((1, 417), (2, 417), (16, 417), (1, 1200), (64, 60)):
                add(f"plan/{preset}/{m}_b{B}_f{frames}", preset, B=B, frames=frames, matrix=m)
        for kvs in knobs:
            for B, ids in ((1, 128), (1, 16), (2, 64), (16, 128)):
                add(f"plan/{preset}/{tag(kvs)}_b{B}_i{ids}", preset, B=B, ids=ids, frames=417, env=env(kvs))
    for kind in STREAMS:
        add(f"plan/medium/{kind}", "medium", B=1 if kind == "stream" else 4, frames=417, kind=kind)
    for preset in ("tiny", "tiny-high", "tiny-ms", "tiny192", "tiny192-ms"):
        add(f"exec/{preset}/b1", preset, ids=21)
        add(f"exec/{preset}/b3", preset, B=3, ids=21)
        for m in MATRIX[1:]:
            add(f"exec/{preset}/{m}", preset, ids=21, matrix=m)
        for kvs in knobs:
            add(f"exec/{preset}/{tag(kvs)}", preset, ids=21, env=env(kvs))
        for kind in STREAMS:
            add(f"exec/{preset}/{kind}", preset, B=1 if kind == "stream" else 3, ids=21, kind=kind)
    for preset in ("tiny192", "tiny192-ms"):
        for forced in FORCED:
            for kvs in [()] + [kvs for kvs in knobs if kvs[0][0] in ("CHAIN_RS", "WN_COMPOSE")]:
                add(f"exec/{preset}/frames{'_'.join(map(str, forced))}{'_' if kvs else ''}{tag(kvs)}", preset, B=len(forced),
                    forced=forced, env=env(kvs))
    return out


def run_case(case, out, root):
    """Child process: the case's calls on the emulator library of `root`."""
    sys.path.insert(0, root)
    import numpy as np
    from piper_amd import _lib as L, weights as W
    from piper_amd.engine import Engine, Timing
    cfg = W.preset("tiny", **WIDE[case["preset"]]) if case["preset"] in WIDE else W.preset(case["preset"])
    eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), lib=L.bind(os.path.join(root, "tests", "emu", "libpiper_hip_emu.so")))
    eng.set_seed(77)
    eng.profile_enable(2)
    B, plan = case["B"], case["frames"] is not None
    # ragged batches: utterance i has ids - 3 * (i % 4) ids
    ids = [W.synthetic_phoneme_ids(max(4, case["ids"] - 3 * (i % 4)), i, id_max=cfg.n_vocab - 1) for i in range(B)]
    sids = [i % cfg.n_speakers for i in range(B)] if cfg.n_speakers > 1 else None
    timing = None
    if case["forced"]:      # exactly F frames per utterance, through the timing plan: two ids (one frame, the rest)
        timing = Timing(durations=[[1, F - 1] for F in case["forced"]])
        ids = [s[:2] for s in ids]
    launches, audio, pcm, durs = [], [], [], []

    def keep(a, p):
        if not plan:
            audio.append(np.asarray(a, np.float32).ravel())
            pcm.append(np.asarray(p, np.int16).ravel())

    if case["kind"] == "call":
        eng.upload(ids, SCALES, sids=sids, timing=timing)
        for _ in range(2):
            eng.run()
            launches.append(eng.run_launches)
            if not plan:
                r = eng.fetch()
                for a, p in zip(r.audio, r.pcm):
                    keep(a, p)
                durs.append(np.asarray(eng.durations(), np.int32).ravel())
    elif case["kind"] == "stream":
        for _ in range(2):
            a, p = next(eng.stream(ids[0], SCALES, sid=None if sids is None else sids[0], chunk_frames=8 if not plan else 45))
            launches.append(eng.run_launches)
            keep(a, p)
    elif case["kind"] == "stream_batch":
        for _ in range(2):
            item = next(eng.stream_batch(ids, SCALES, sids=sids, chunk_frames=8 if not plan else 45))
            launches.append(eng.run_launches)
            for a, p in item:
                keep(a, p)
    else:
        with eng.stream_pool(B + 1, 4096) as pool:
            pool.join(ids[:1], SCALES, sids=None if sids is None else sids[:1])
            for k in range(2):
                got = pool.next(8 if not plan else 45)
                launches.append(eng.run_launches)
                for s in sorted(got):
                    keep(*got[s])
                if k == 0 and B > 1:
                    pool.join(ids[1:], SCALES, sids=None if sids is None else sids[1:])
    rows = [{"name": r["name"], "launches": int(r["launches"]), "flops": float(r["flops"]), "bytes": float(r["bytes"])}
            for r in eng.profile() if r["launches"]]
    eng.close()
    with open(os.path.join(out, "rows.json"), "w") as f:
        json.dump(rows, f, indent=0, sort_keys=True)
    with open(os.path.join(out, "launches.txt"), "w") as f:
        f.write(" ".join(str(int(n)) for n in launches) + "\n")
    if not plan:
        np.concatenate(audio).tofile(os.path.join(out, "audio.f32"))
        np.concatenate(pcm).tofile(os.path.join(out, "pcm.i16"))
        np.concatenate(durs or [np.zeros(0, np.int32)]).tofile(os.path.join(out, "durations.i32"))


def spawn(case, out_root, root, base_env):
    out = os.path.join(out_root, case["name"])
    os.makedirs(out)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("PIPER_HIP_", "EMU_"))}
    env.update(base_env)
    env.update(case["env"], EMU_PLAN_TRACE=os.path.join(out, "trace.txt"), PIPER_HIP_MATRIX=case["matrix"])
    if case["frames"] is not None:
        env.update(EMU_PLAN_ONLY="1", EMU_PLAN_FRAMES=str(case["frames"]))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", json.dumps(case), "--root", root, out],
                         env=env, capture_output=True, text=True)
    return case["name"], res.returncode, res.stderr[-2000:]


def tree_sha256(top):
    h = hashlib.sha256()
    for d, dirs, files in os.walk(top):
        dirs.sort()
        for fn in sorted(files):
            p = os.path.join(d, fn)
            h.update(os.path.relpath(p, top).encode() + b"\0")
            with open(p, "rb") as f:
                h.update(f.read())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("out")
    ap.add_argument("--root", default=HERE, help="checkout whose piper_amd package and emulator library run the cases")
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--only", default="", help="run only the cases whose name starts with this")
    ap.add_argument("--env", action="append", default=[], metavar="KNOB=VALUE",
                    help="a policy knob set for every case, under the case's own settings (e.g. PIPER_HIP_WN_COMPOSE=0: the "
                         "tree of a parent that has no such knob)")
    ap.add_argument("--case", help=argparse.SUPPRESS)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    if a.case:
        run_case(json.loads(a.case), a.out, root)
        return 0
    todo = [c for c in cases() if c["name"].startswith(a.only)]
    if os.path.isdir(a.out) and os.listdir(a.out):
        ap.error(f"{a.out} is not empty")
    os.makedirs(a.out, exist_ok=True)
    with ThreadPoolExecutor(max(1, min(a.jobs, 16))) as pool:
        done = list(pool.map(lambda c: spawn(c, a.out, root, dict(kv.split("=", 1) for kv in a.env)), todo))
    bad = [(n, rc, err) for n, rc, err in done if rc]
    for n, rc, err in bad:
        print(f"FAILED {n} (exit {rc})\n{err}", file=sys.stderr)
    traced = 0
    for c in todo:
        t = os.path.join(a.out, c["name"], "trace.txt")
        if os.path.exists(t):
            with open(t) as f:
                traced += sum(1 for _ in f)
    print(json.dumps({"cases": len(todo), "failed": len(bad), "launches_traced": traced, "sha256": tree_sha256(a.out)}))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
