"""What the output-rate conversion costs (pe_set_output_rate, kernels/resample.h), measured on the GPU with the timing of
bench.py's legs: a step = ids from host memory (pe_upload), the device pipeline with both noise sites drawn by the engine
(pe_run), int16 PCM in host memory (pe_fetch, which ends in a stream synchronisation); W untimed steps, then K timed ones
between two device synchronisations.

Two legs -- one utterance of the medium voice, 64 utterances of the high voice, 128 ids each -- at the native rate, at 8000
and at 48000 Hz, in one process; then, with the level-2 profile on, the row of resample_kernel: time per launch, its
algorithmic bytes (every native sample in once, every output out once) and the bytes/s that makes, next to a plain
device-to-device copy of the same number of bytes. One JSON object per line.

    python scripts/resample_cost.py                    # all of it
    python scripts/resample_cost.py --native-only      # needs nothing of the rate API: also runs on earlier commits
    python scripts/resample_cost.py --root DIR ...     # import piper_amd from DIR (another checkout, built)
"""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--native-only", action="store_true")
    ap.add_argument("--steps1", type=int, default=300, help="timed steps of the one-utterance leg")
    ap.add_argument("--steps64", type=int, default=30, help="timed steps of the 64-utterance leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    from piper_amd import weights as W
    from piper_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("resample_cost.py measures on the GPU and found none")

    def leg(preset, B, T, steps):
        cfg = W.preset(preset)
        eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
        id_max = min(cfg.n_vocab - 1, 129)
        ids = [W.synthetic_phoneme_ids(T, i, id_max=id_max) for i in range(B)]
        host_in = eng.pack_host(ids, (0.667, 1.0, 0.8))

        def step():
            eng.upload_host(host_in)
            eng.run()
            return eng.fetch_views(False, True)

        rates = [0] if args.native_only else [0, 8000, 48000, 0]       # (native twice: the spread within the process)
        for rate in rates:
            if not args.native_only:
                eng.set_output_rate(rate)
            eng.set_seed(1234)
            for _ in range(args.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            samples = 0
            for _ in range(steps):
                samples += step().sample_offsets[B]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            out = {"tag": args.tag, "leg": f"{preset} x {B}", "ids": T, "rate": rate or cfg.sample_rate,
                   "native": rate == 0, "steps": steps, "ms_per_step": dt / steps * 1e3,
                   "samples_per_s": samples / dt, "launches": eng.run_launches}
            print(json.dumps(out), flush=True)
        if not args.native_only:
            for rate in (8000, 48000):
                eng.set_output_rate(rate)
                eng.set_seed(1234)
                for _ in range(3):
                    step()
                eng.profile_enable(2)
                eng.profile_reset()
                n = 10
                for _ in range(n):
                    step()
                rows = {r["name"]: r for r in eng.profile()}
                eng.profile_enable(0)
                r = rows["resample_kernel"]
                per_ms, per_bytes = r["ms"] / r["launches"], r["bytes"] / r["launches"]
                # a plain copy that moves the same bytes (half read, half written)
                nel = max(1, int(per_bytes / 8))
                src, dst = torch.empty(nel, dtype=torch.float32, device="cuda"), torch.empty(nel, dtype=torch.float32, device="cuda")
                for _ in range(5):
                    dst.copy_(src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                copy_ms = e0.elapsed_time(e1) / 20
                print(json.dumps({"tag": args.tag, "leg": f"{preset} x {B}", "rate": rate, "row": "resample_kernel",
                                  "launches": r["launches"], "ms_per_launch": per_ms, "bytes_per_launch": per_bytes,
                                  "GB_per_s": per_bytes / per_ms / 1e6, "copy_ms_same_bytes": copy_ms,
                                  "copy_GB_per_s": per_bytes / copy_ms / 1e6,
                                  "rows_ms_per_launch": rows["resample_rows_kernel"]["ms"] / rows["resample_rows_kernel"]["launches"]}),
                      flush=True)
        eng.close()

    leg("medium", 1, 128, args.steps1)
    leg("high", 64, 128, args.steps64)


if __name__ == "__main__":
    main()
