"""What the look-ahead limiter costs (pe_set_loudness_limiter, kernels/limiter.h), measured on the GPU with the timing of
bench.py's legs: a step = ids from host memory (pe_upload), the device pipeline with both noise sites drawn by the engine
(pe_run), int16 PCM in host memory (pe_fetch, which ends in a stream synchronisation); W untimed steps, then K timed ones
between two device synchronisations.

Two legs -- one utterance of the medium voice, 64 utterances of the high voice, 128 ids each -- with the target loudness on
(a target high enough that the ceiling conflicts, so rows are shaped) and the limiter off, on and off again under the
sample-peak ceiling, then off, on and off again under the true-peak ceiling, at the native rate and at 48000 Hz, in one
process; then, with the level-2 profile on, the rows of the stage's kernels under either ceiling. One JSON object per line.

    python scripts/limiter_cost.py                   # all of it
    python scripts/limiter_cost.py --off-only        # needs nothing of the limiter's API: also runs on the parent commit
    python scripts/limiter_cost.py --root DIR ...    # import piper_amd from DIR (another checkout, built)
"""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--steps1", type=int, default=300, help="timed steps of the one-utterance leg")
    ap.add_argument("--steps64", type=int, default=30, help="timed steps of the 64-utterance leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--target", type=float, default=-8.0)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    from piper_amd import weights as W
    from piper_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("limiter_cost.py measures on the GPU and found none")

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

        def setting(true_peak, limiter):
            if args.off_only:
                eng.set_loudness(args.target, -1.0, true_peak=true_peak)
            else:
                eng.set_loudness(args.target, -1.0, true_peak=true_peak, limiter=limiter, limiter_ms=args.window_ms)

        for rate in (0, 48000):
            eng.set_output_rate(rate)
            # (off twice under the sample-peak ceiling: the spread within the process)
            for tp, lim in ([(False, False), (False, False), (True, False)] if args.off_only else
                            [(False, False), (False, True), (False, False), (True, False), (True, True), (True, False)]):
                setting(tp, lim)
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
                L, scale, peak, flags = eng.last_loudness()
                out = {"tag": args.tag, "leg": f"{preset} x {B}", "ids": T, "rate": rate or cfg.sample_rate, "true_peak": tp,
                       "limiter": lim, "steps": steps, "ms_per_step": dt / steps * 1e3, "samples_per_s": samples / dt,
                       "launches": eng.run_launches, "scale": [round(float(v), 1) for v in scale[:4]],
                       "flags": [int(v) for v in flags[:4]]}
                if lim:
                    red, cnt, _ = eng.last_limiter()
                    out["max_reduction"] = [round(float(v), 4) for v in red[:4]]
                    out["shaped_samples"] = [int(v) for v in cnt[:4]]
                    out["trim"] = [round(float(v), 6) for v in eng.last_limiter()[2][:4]]
                print(json.dumps(out), flush=True)
            if args.off_only:
                continue
            for tp, names in ((False, ("loudness_seg_kernel", "loudness_gain_kernel", "limiter_kernel")),
                              (True, ("loudness_seg_kernel", "true_peak_v_kernel", "loudness_gain_kernel", "limiter_true_kernel",
                                      "true_peak_kernel", "pcm16_trim_kernel"))):
                setting(tp, True)
                eng.set_seed(1234)
                for _ in range(3):
                    step()
                eng.profile_enable(2)
                eng.profile_reset()
                for _ in range(10):
                    step()
                rows = {r["name"]: r for r in eng.profile() if r["launches"] > 0}
                eng.profile_enable(0)
                row = {"tag": args.tag, "leg": f"{preset} x {B}", "rate": rate or cfg.sample_rate, "true_peak": tp,
                       "row": "profile level 2"}
                for name in names:
                    r = rows[name]
                    row[name] = {"us_per_launch": r["ms"] / r["launches"] * 1e3, "bytes_per_launch": r["bytes"] / r["launches"]}
                print(json.dumps(row), flush=True)
        eng.close()

    leg("medium", 1, 128, args.steps1)
    leg("high", 64, 128, args.steps64)


if __name__ == "__main__":
    main()
