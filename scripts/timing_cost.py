"""What a timing plan costs and what an all-forced call saves (pe_timing, kernels/timing.h), measured on the GPU with the
timing of bench.py's legs: a step = inputs from host memory (pe_upload / pe_upload_timed), the device pipeline with the
engine's own noise (pe_run), int16 PCM in host memory (pe_fetch, which ends in a stream synchronisation); W untimed steps,
then K timed ones between two device synchronisations. One JSON object per line.

  kernel   level-2 profile rows (event-timed, graphs off) of duration_kernel and duration_plan_kernel -- plain plan, target,
           target at 8192 ids -- at the medium voice's one-utterance shape and at batch 64, with the stage-A time (rows
           text_encoder + duration_predictor) of the same calls
  saving   the untimed step against the step with every duration forced (the durations of an untimed call fed back):
           medium and high voice, one utterance and batch 64. The timed step runs as A, read-back, B; the untimed
           one-utterance step is the speculative one-graph form, and with PIPER_HIP_SPEC=0 the two-graph form.

    python scripts/timing_cost.py [--what kernel|saving|all]
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="all", choices=("kernel", "saving", "all"))
    ap.add_argument("--steps1", type=int, default=200)
    ap.add_argument("--steps64", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from piper_amd import weights as W
    from piper_amd.engine import Engine, Timing
    if not torch.cuda.is_available():
        raise SystemExit("timing_cost.py measures on the GPU and found none")

    def engine(preset, spec=True):
        if spec:
            os.environ.pop("PIPER_HIP_SPEC", None)
        else:
            os.environ["PIPER_HIP_SPEC"] = "0"
        cfg = W.preset(preset)
        eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
        os.environ.pop("PIPER_HIP_SPEC", None)
        return cfg, eng

    def texts(cfg, B, T):
        return [W.synthetic_phoneme_ids(T, i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(B)]

    def kernel_rows(preset, B, T, plans, n=5):
        cfg, eng = engine(preset)
        ids = texts(cfg, B, T)
        nat = eng.synthesize_batch(ids).frames
        for name in plans:
            timing = None
            if name == "plain plan":
                timing = Timing()
            elif name == "target":
                timing = Timing(target_frames=[min(60000, int(1.2 * f) + 1) for f in nat])
            packed = eng.pack_host(ids, (0.667, 1.0, 0.8), timing=timing)
            for _ in range(2):
                eng.upload_host(packed); eng.run(); eng.fetch_views(False, True)
            eng.profile_enable(2)
            eng.profile_reset()
            for _ in range(n):
                eng.upload_host(packed); eng.run(); eng.fetch_views(False, True)
            prof = eng.profile()
            eng.profile_enable(0)
            rows = {r["name"]: r for r in prof if r["launches"]}
            k = rows["duration_kernel" if timing is None else "duration_plan_kernel"]
            stage_a = (prof[0]["ms"] + prof[1]["ms"]) / n
            us = k["ms"] / k["launches"] * 1e3
            print(json.dumps({"what": "kernel", "leg": f"{preset} x {B}", "ids": T, "plan": name, "kernel": k["name"],
                              "us_per_launch": us, "stage_a_ms": stage_a, "share_of_stage_a": us / 1e3 / stage_a}), flush=True)
        eng.close()

    def timed_steps(eng, packed, B, steps):
        for _ in range(args.warmup):
            eng.upload_host(packed); eng.run(); eng.fetch_views(False, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            eng.upload_host(packed); eng.run(); eng.fetch_views(False, True)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, eng.run_launches

    def saving(preset, B, T, steps):
        for spec in ((True, False) if B == 1 else (True,)):
            cfg, eng = engine(preset, spec)
            ids = texts(cfg, B, T)
            eng.set_seed(1234)
            eng.synthesize_batch(ids)
            d = eng.durations()
            offs = np.concatenate([[0], np.cumsum([len(s) for s in ids])])
            forced = Timing(durations=[d[offs[b]:offs[b + 1]] for b in range(B)])
            plain, timed = eng.pack_host(ids, (0.667, 1.0, 0.8)), eng.pack_host(ids, (0.667, 1.0, 0.8), timing=forced)
            series = {"untimed": [], "all forced": []}
            launches = {}
            for _ in range(3):                             # alternating, so that drift shows up in both
                for name, packed in (("untimed", plain), ("all forced", timed)):
                    ms, launches[name] = timed_steps(eng, packed, B, steps)
                    series[name].append(round(ms, 4))
            form = "two-graph (PIPER_HIP_SPEC=0)" if not spec else ("speculative one-graph" if B <= 4 else "two-graph")
            print(json.dumps({"what": "saving", "leg": f"{preset} x {B}", "ids": T, "untimed_form": form,
                              "untimed_ms": series["untimed"], "all_forced_ms": series["all forced"], "launches": launches,
                              "speculation": eng.speculation_stats}), flush=True)
            eng.close()

    if args.what in ("kernel", "all"):
        kernel_rows("medium", 1, 128, ("untimed", "plain plan", "target"))
        kernel_rows("medium", 64, 128, ("untimed", "plain plan", "target"))
        kernel_rows("medium", 1, 8192, ("untimed", "target"), n=2)
    if args.what in ("saving", "all"):
        for preset in ("medium", "high"):
            saving(preset, 1, 128, args.steps1)
            saving(preset, 64, 128, args.steps64)


if __name__ == "__main__":
    main()
