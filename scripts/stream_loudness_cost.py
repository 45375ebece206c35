"""What a stream at a target loudness costs per chunk (pe_set_stream_loudness, kernels/stream_loudness.h), measured on the GPU
against the running-peak mode of pe_set_stream_gain, after the pattern of scripts/stream_gain_cost.py.

The flagship stream: the high voice, 64 utterances x 128 ids begun together (--batch 1: one row), chunks of 45 frames, int16
only. A timed call is one pe_stream_next_batch through ctypes (it ends in a stream synchronisation), and only the chunks every
utterance still takes part in with a whole chunk are counted. The duration noise is injected, so every stream has the same
frame counts; the prior noise is the engine's, so every stage is a captured graph.

The legs alternate inside one process, round after round: running, loudness, chunk, running again. The second running leg is
the A/A figure: the range of the per-round p50s of both says what this process can resolve. There is no pass / fail threshold
on the time. The launch counts come from one profiled stream per mode. One JSON object per line, the verdict last.

    python scripts/stream_loudness_cost.py                  # all four legs, 64 rows
    python scripts/stream_loudness_cost.py --batch 1        # one row
    python scripts/stream_loudness_cost.py --running-only   # needs nothing of the loudness API: also runs on the parent commit
    python scripts/stream_loudness_cost.py --root DIR ...   # import piper_amd from DIR (another checkout, built)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--running-only", action="store_true", help="needs nothing of the loudness API: also runs on the parent commit")
    ap.add_argument("--rounds", type=int, default=6, help="streams per leg (after one untimed round)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ids", type=int, default=128)
    ap.add_argument("--preset", default="high")
    ap.add_argument("--chunk-frames", type=int, default=45)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    from piper_amd import _lib as L, weights as W
    from piper_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("stream_loudness_cost.py measures on the GPU and found none")

    cfg = W.preset(args.preset)
    eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
    lib, h = eng._lib, eng._h
    B, T, cf = args.batch, args.ids, args.chunk_frames
    ids = [W.synthetic_phoneme_ids(T, 60 + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(B)]
    nw = np.random.default_rng(64).standard_normal((B, 2, T)).astype(np.float32)
    flat, offs = eng._pack(ids)
    scales = np.ascontiguousarray(np.tile(np.asarray((0.667, 1.0, 0.8), np.float32), (B, 1)))
    p64, pf, p32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def stream():
        """One stream to its end; seconds per call for the calls in which every utterance delivers a whole chunk."""
        keep = []
        nref = eng._noise(nw, None, keep)
        frames, halo = np.zeros(B, np.int32), C.c_int32()
        eng._check(lib.pe_stream_begin_batch(h, flat.ctypes.data_as(p64), offs.ctypes.data_as(p64), B, scales.ctypes.data_as(pf),
                                             None, nref, frames.ctypes.data_as(p32), C.byref(halo)))
        whole = int(frames.min()) // cf
        ch = L.PeStreamChunk()
        times, k = [], 0
        while True:
            t0 = time.perf_counter()
            rc = lib.pe_stream_next_batch(h, cf, 0, C.byref(ch))
            dt = time.perf_counter() - t0
            eng._check(rc)
            if ch.sample_offsets[B] == 0:
                return times, frames
            if k < whole:
                times.append(dt)
            k += 1

    legs = [("running", "running")] if args.running_only else [("running", "running"), ("loudness", "loudness"), ("chunk", "chunk"),
                                                               ("running", "running (A/A)")]

    def set_mode(mode):
        if mode == "loudness":
            eng.set_stream_loudness(-19.0, -1.0, None, 5.0)
        else:
            eng.set_stream_gain(mode, 0.0, 5.0)

    def launches(mode):
        """Kernel launches of one whole-chunk call (level-2 profile rows of one stream, divided by its calls)."""
        set_mode(mode)
        eng.profile_enable(2)
        eng.profile_reset()
        t, fr = stream()
        rows = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
        eng.profile_enable(0)
        calls = -(-int(fr.max()) // cf)
        tail = {n: v for n, v in rows.items() if n.startswith(("chunk_", "stream_"))}
        return {"mode": mode, "calls": calls, "launches_per_call": sum(rows.values()) / calls, "delivery_launches": tail}

    per_leg = {name: [] for _, name in legs}
    frames = None
    for rnd in range(args.rounds + 1):
        for mode, name in legs:
            set_mode(mode)
            t, frames = stream()
            if rnd:                                      # round 0 captures the graphs
                per_leg[name].append(t)
    captures = eng.graph_stats[1]
    for mode, name in legs:                              # ... and a steady server captures no more
        set_mode(mode)
        stream()
    assert eng.graph_stats[1] == captures, (captures, eng.graph_stats)
    for mode in sorted({m for m, _ in legs}):
        print(json.dumps({"tag": args.tag, "batch": B, **launches(mode)}), flush=True)
    set_mode("chunk")

    def p50(x):
        return float(np.median(np.asarray(x))) * 1e3

    out = {}
    for _, name in legs:
        rounds = per_leg[name]
        allt = [v for r in rounds for v in r]
        out[name] = {"p50_ms": p50(allt), "p10_ms": float(np.percentile(allt, 10)) * 1e3,
                     "p90_ms": float(np.percentile(allt, 90)) * 1e3, "round_p50_ms": [p50(r) for r in rounds],
                     "calls": len(allt)}
        print(json.dumps({"tag": args.tag, "leg": name, "voice": args.preset, "batch": B, "ids": T, "chunk_frames": cf,
                          "frames_min": int(frames.min()), "frames_max": int(frames.max()), **out[name]}), flush=True)
    if not args.running_only:
        aa = out["running"]["round_p50_ms"] + out["running (A/A)"]["round_p50_ms"]
        spread = max(aa) - min(aa)
        base = out["running"]["p50_ms"]
        verdict = {"tag": args.tag, "aa_p50_delta_ms": out["running (A/A)"]["p50_ms"] - base, "aa_round_p50_range_ms": spread,
                   "loudness_minus_running_ms": out["loudness"]["p50_ms"] - base,
                   "chunk_minus_running_ms": out["chunk"]["p50_ms"] - base, "graph_captures": captures}
        print(json.dumps(verdict), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
