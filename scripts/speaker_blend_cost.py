"""What a speaker blend costs (pe_upload_blended, kernels/glue.h: speaker_blend_kernel), measured on the GPU with the timing of
bench.py's legs: a step = inputs from host memory (pe_upload / pe_upload_blended on arrays packed once), the device pipeline
with both noise sites drawn by the engine (pe_run), int16 PCM in host memory (pe_fetch, which ends in a stream
synchronisation); W untimed steps, then K timed ones between two device synchronisations.

A multi-speaker medium voice (16 speakers, gin 512), 128 ids per utterance, one utterance and 64, each with plain speaker
ids and with 8-component blends whose vector equals the plain id's row (one weight 1, seven weights 0: every component is
read, and both kinds synthesize the same frames -- a blend that changes the voice changes the durations and with them the
work of the whole call, which is not what the blend costs). The kinds alternate, plain first, for --rounds rounds in one process: the figure of a kind
is the median of its rounds, its spread their range -- the plain rounds against each other are the run-to-run spread that a
difference has to exceed to mean anything. One JSON object per line, and a table between the marker lines of --out.

    python scripts/speaker_blend_cost.py                                   # all of it, table to profiles/speaker_blend.md
    python scripts/speaker_blend_cost.py --plain-only --out FILE           # needs nothing of the blend API: also runs on earlier commits
    python scripts/speaker_blend_cost.py --root DIR ...                    # import piper_amd from DIR (another checkout, built)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=here)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--steps1", type=int, default=400, help="timed steps per round of the one-utterance leg")
    ap.add_argument("--steps64", type=int, default=30, help="timed steps per round of the 64-utterance leg")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(here, "profiles", "speaker_blend.md"))
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    from piper_amd import weights as W
    from piper_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("speaker_blend_cost.py measures on the GPU and found none")

    cfg = W.preset("medium", n_speakers=16, gin=512)
    eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    lib = eng._lib
    id_max = min(cfg.n_vocab - 1, 129)
    rng = np.random.default_rng(9)
    table = []

    def leg(B, T, steps):
        ids = [W.synthetic_phoneme_ids(T, i, id_max=id_max) for i in range(B)]
        flat, offs = eng._pack(ids)
        i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
        per = np.ascontiguousarray(np.tile(np.asarray((0.667, 1.0, 0.8), np.float32), (B, 1)))
        sids = np.ascontiguousarray(rng.integers(cfg.n_speakers, size=B), np.int64)
        head = (eng._h, flat.ctypes.data_as(i64p), offs.ctypes.data_as(i64p), B, per.ctypes.data_as(f32p))
        keep = []
        blend = None
        if not args.plain_only:
            from piper_amd.engine import pack_speakers
            # like for like: utterance b's blend is (its plain id, 1.0) and seven more rows at weight 0.0 -- all eight are
            # read and walked, and g is bit for bit the plain call's, so both kinds synthesize the same frames
            speakers = [[(int(sids[u]), 1.0)] + [(int(s), 0.0) for s in rng.integers(cfg.n_speakers, size=7)] for u in range(B)]
            _, blend = pack_speakers(speakers, None, B, cfg.gin, keep)

        def step(kind):
            if kind == "plain":
                eng._check(lib.pe_upload_scaled(*head, sids.ctypes.data_as(i64p), None))
            else:
                eng._check(lib.pe_upload_blended(*head, None, None, None, None, blend))
            eng.run()
            return eng.fetch_views(False, True)

        kinds = ["plain"] if args.plain_only else ["plain", "blend"]
        ms = {k: [] for k in kinds}
        launches = {}
        for _ in range(args.rounds):
            for kind in kinds:
                eng.set_seed(1234)
                for _ in range(args.warmup):
                    step(kind)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(kind)
                torch.cuda.synchronize()
                ms[kind].append((time.perf_counter() - t0) / steps * 1e3)
                launches[kind] = eng.run_launches
        for kind in kinds:
            row = {"tag": args.tag, "leg": f"medium-ms x {B}", "ids": T, "kind": kind, "steps": steps, "rounds": args.rounds,
                   "ms_per_step": [round(v, 5) for v in ms[kind]], "median_ms": statistics.median(ms[kind]),
                   "spread_ms": max(ms[kind]) - min(ms[kind]), "launches": launches[kind]}
            print(json.dumps(row), flush=True)
            table.append(row)

    leg(1, 128, args.steps1)
    leg(64, 128, args.steps64)
    eng.close()

    lines = ["| leg | kind | median ms / step | range over rounds (ms) | launches |", "|---|---|---|---|---|"]
    for r in table:
        lines.append(f"| {r['leg']} | {r['kind']} | {r['median_ms']:.4f} | {min(r['ms_per_step']):.4f} .. {max(r['ms_per_step']):.4f} | {r['launches']} |")
    if not args.plain_only:
        lines += ["", "| leg | blend - plain (us / step) | of the plain step | plain spread (us) |", "|---|---|---|---|"]
        for p, b in zip(table[0::2], table[1::2]):
            d = b["median_ms"] - p["median_ms"]
            lines.append(f"| {p['leg']} | {d * 1e3:+.2f} | {d / p['median_ms'] * 100:+.3f} % | {p['spread_ms'] * 1e3:.2f} |")
    text = f"steps per round {args.steps1} / {args.steps64}, warm-up {args.warmup}, rounds {args.rounds}, tag {args.tag!r}\n\n" + "\n".join(lines) + "\n"
    print(text)
    if args.out:
        # the figures go between two marker lines of the file; what is written around them stays
        begin, end = "<!-- figures: scripts/speaker_blend_cost.py -->\n", "<!-- end of figures -->\n"
        old = open(args.out, encoding="utf-8").read() if os.path.exists(args.out) else "# What a speaker blend costs\n\n" + begin + end
        if begin not in old or end not in old:
            old += "\n" + begin + end
        i, j = old.index(begin) + len(begin), old.index(end)
        with open(args.out, "w", encoding="utf-8") as f:
            f.write(old[:i] + text + old[j:])


if __name__ == "__main__":
    main()
