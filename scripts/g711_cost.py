"""What G.711 delivery costs (pe_set_sample_format, kernels/g711.h), measured on the GPU with the timing of bench.py's legs: a
step = ids from host memory (pe_upload), the device pipeline with both noise sites drawn by the engine (pe_run), the result
in host memory (pe_fetch, which ends in a stream synchronisation); W untimed steps, then K timed ones between two device
synchronisations.

Two whole-utterance legs -- one utterance of the medium voice, 64 utterances of the high voice, 128 ids each: the step time
with s16 on this commit and on the parent commit (piper_amd/libab_base.so, which scripts/build_base.sh builds), so that "off
costs nothing" is a comparison against the parent and not against itself; the step time with ulaw; the encoder's own kernel
time from the level-2 profile. Every timed setting runs --repeats times and the spread is reported beside the median. Then a
pool of 64 listeners of the medium voice: the time per chunk call with and without a law. One JSON object per line; the
table goes into profiles/g711.md.

    scripts/build_base.sh HEAD~1 && python scripts/g711_cost.py
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps1", type=int, default=200, help="timed steps of the one-utterance leg")
    ap.add_argument("--steps64", type=int, default=20, help="timed steps of the 64-utterance leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "g711.md"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from piper_amd import _lib as L, weights as W
    from piper_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("g711_cost.py measures on the GPU and found none")

    class ParentLib(C.CDLL):
        """The parent commit's library has none of this commit's symbols: they become stubs that fail when called."""
        def __getattr__(self, name):
            try:
                return super().__getattr__(name)
            except AttributeError:
                if not name.startswith("pe_"):
                    raise
                stub = C.CFUNCTYPE(C.c_int)(lambda *a: 1)
                setattr(self, name, stub)
                return stub

    libs = [("this commit", L.get_lib())]
    base = os.path.join(ROOT, "piper_amd", "libab_base.so")
    if os.path.exists(base):
        cdll, L.C.CDLL = L.C.CDLL, ParentLib
        try:
            libs.append(("parent commit", L.bind(base)))
        finally:
            L.C.CDLL = cdll
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(step, steps):
        out = []
        for _ in range(args.repeats):
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / steps * 1e3)
        return statistics.median(out), max(out) - min(out)

    def leg(preset, B, T, steps):
        cfg = W.preset(preset)
        blob = W.pack_blob(cfg, W.synthetic_weights(cfg, 1234))
        id_max = min(cfg.n_vocab - 1, 129)
        ids = [W.synthetic_phoneme_ids(T, i, id_max=id_max) for i in range(B)]
        for who, lib in libs:
            eng = Engine(blob=blob, device=0, lib=lib)
            host_in = eng.pack_host(ids, (0.667, 1.0, 0.8))

            def step():
                eng.upload_host(host_in)
                eng.run()
                return eng.fetch_views(False, True)

            for fmt in (("s16", "ulaw", "alaw") if who == "this commit" else ("s16",)):
                if who == "this commit":
                    eng.set_sample_format(fmt)
                eng.set_seed(1234)
                ms, spread = timed(step, steps)
                emit({"leg": f"{preset} x {B}", "library": who, "format": fmt, "ms_per_step": ms, "spread_ms": spread,
                      "launches": eng.run_launches})
            if who == "this commit":
                eng.set_sample_format("ulaw")
                for _ in range(3):
                    step()
                eng.profile_enable(2)
                eng.profile_reset()
                for _ in range(10):
                    step()
                prof = {r["name"]: r for r in eng.profile() if r["launches"] > 0}
                eng.profile_enable(0)
                r = prof["g711_kernel"]
                emit({"leg": f"{preset} x {B}", "library": who, "row": "g711_kernel", "us_per_launch": r["ms"] / r["launches"] * 1e3,
                      "bytes_per_launch": r["bytes"] / r["launches"]})
            eng.close()

    def pool_leg(preset, slots, T, chunk):
        cfg = W.preset(preset)
        eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
        id_max = min(cfg.n_vocab - 1, 129)
        ids = [W.synthetic_phoneme_ids(T, i, id_max=id_max) for i in range(slots)]
        for fmt in ("s16", "ulaw", "s16", "ulaw"):
            eng.set_sample_format(fmt)
            eng.set_seed(1234)
            with eng.stream_pool(slots, 2048) as pool:
                pool.join(ids, (0.667, 1.0, 0.8))
                full = int(np.min(pool.frames)) // chunk      # calls in which every slot delivers a whole chunk
                times = []
                for k in range(full):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pool.next(chunk, want_audio=False)
                    times.append((time.perf_counter() - t0) * 1e3)
                while pool.next(chunk, want_audio=False):
                    pass
            t = times[2:] or times
            emit({"leg": f"pool of {slots}, {preset}, chunks of {chunk} frames", "format": fmt, "calls": len(t),
                  "ms_per_chunk": statistics.median(t), "spread_ms": max(t) - min(t)})
        eng.close()

    leg("medium", 1, 128, args.steps1)
    leg("high", 64, 128, args.steps64)
    pool_leg("medium", 64, 128, 45)

    with open(args.out, "w", encoding="utf-8") as f:
        f.write("# G.711 delivery: what it costs\n\n"
                "Written by `scripts/g711_cost.py` on an MI355X (its docstring says what a step is). `spread` is the largest\n"
                "minus the smallest of the repeats of one setting in one process: differences below it say nothing.\n\n"
                "## Whole utterances\n\n| leg | library | format | ms per step | spread | launches |\n|---|---|---|---|---|---|\n")
        for r in rows:
            if "ms_per_step" in r:
                f.write(f"| {r['leg']} | {r['library']} | {r['format']} | {r['ms_per_step']:.4f} | {r['spread_ms']:.4f} | {r['launches']} |\n")
        f.write("\n## The encoder's own kernel (level-2 profile, ulaw)\n\n| leg | us per launch | bytes per launch |\n|---|---|---|\n")
        for r in rows:
            if r.get("row") == "g711_kernel":
                f.write(f"| {r['leg']} | {r['us_per_launch']:.2f} | {r['bytes_per_launch']:.0f} |\n")
        f.write("\n## Pool chunk\n\n| leg | format | calls | ms per chunk (median) | spread |\n|---|---|---|---|---|\n")
        for r in rows:
            if "ms_per_chunk" in r:
                f.write(f"| {r['leg']} | {r['format']} | {r['calls']} | {r['ms_per_chunk']:.4f} | {r['spread_ms']:.4f} |\n")
        if len(libs) == 1:
            f.write("\nThe parent commit's library was not there (scripts/build_base.sh): no comparison against the parent.\n")


if __name__ == "__main__":
    main()
