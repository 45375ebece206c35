"""What the look-ahead limiter on streams costs per chunk (pe_set_stream_limiter, kernels/stream_limiter.h), measured on the GPU on
one build: streams at a target loudness with the limiter off -- unchanged by the limiter's arrival, so it is the reference --
against the same streams with the limiter on, after the pattern of scripts/stream_loudness_cost.py.

The flagship stream: the high voice, 64 utterances x 128 ids begun together (--batch 1: one listener), chunks of 45 frames,
int16 only. A timed call is one pe_stream_next_batch through ctypes (it ends in a stream synchronisation), and only the chunks
every utterance still takes part in with a whole chunk are counted. The time to the first delivered sample is the begin call
plus every chunk call up to the first one that hands out samples (with the limiter a stream holds back 2 W samples: a chunk
shorter than that delivers nothing). The duration noise is injected, so every stream has the same frame counts; the prior noise
is the engine's, so every stage is a captured graph.

The legs alternate inside one process, round after round: off, on, off again. The second off leg is the A/A figure: the range
of the per-round p50s of both says what this process can resolve. There is no pass / fail threshold on the time. The launch
counts come from one profiled stream per leg. One JSON object per line, the verdict last.

    python scripts/stream_limiter_cost.py                   # all three legs, 64 rows
    python scripts/stream_limiter_cost.py --batch 1         # one listener
    python scripts/stream_limiter_cost.py --window-ms 10    # another window
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
    ap.add_argument("--rounds", type=int, default=6, help="streams per leg (after one untimed round)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ids", type=int, default=128)
    ap.add_argument("--preset", default="high")
    ap.add_argument("--chunk-frames", type=int, default=45)
    ap.add_argument("--window-ms", type=float, default=5.0)
    ap.add_argument("--target", type=float, default=-16.0)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    from piper_amd import _lib as L, weights as W
    from piper_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("stream_limiter_cost.py measures on the GPU and found none")

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
        """One stream to its end: seconds per call for the calls in which every utterance delivers a whole chunk, the
        seconds to the first delivered sample, the frame counts and the shaped samples reported."""
        keep = []
        nref = eng._noise(nw, None, keep)
        frames, halo = np.zeros(B, np.int32), C.c_int32()
        t_begin = time.perf_counter()
        eng._check(lib.pe_stream_begin_batch(h, flat.ctypes.data_as(p64), offs.ctypes.data_as(p64), B, scales.ctypes.data_as(pf),
                                             None, nref, frames.ctypes.data_as(p32), C.byref(halo)))
        whole = int(frames.min()) // cf
        calls = -(-int(frames.max()) // cf)
        ch = L.PeStreamChunk()
        times, first, shaped = [], None, 0
        for k in range(calls):
            t0 = time.perf_counter()
            rc = lib.pe_stream_next_batch(h, cf, 0, C.byref(ch))
            t1 = time.perf_counter()
            eng._check(rc)
            if first is None and ch.sample_offsets[B] > 0:
                first = t1 - t_begin
            if k < whole:
                times.append(t1 - t0)
            if eng.stream_limiter()[0]:
                shaped += int(eng.stream_last_limiter()[1].sum())
        eng._check(lib.pe_stream_next_batch(h, cf, 0, C.byref(ch)))      # the call that ends it
        assert ch.sample_offsets[B] == 0
        return times, first, frames, shaped

    legs = [(False, "off"), (True, "on"), (False, "off (A/A)")]

    def set_mode(on):
        eng.set_stream_loudness(args.target, -1.0, None, 5.0, limiter=on, limiter_ms=args.window_ms)

    def launches(on):
        """Kernel launches of one whole-chunk call (level-2 profile rows of one stream, divided by its calls)."""
        set_mode(on)
        eng.profile_enable(2)
        eng.profile_reset()
        t, _, fr, shaped = stream()
        rows = {r["name"]: r["launches"] for r in eng.profile()[5:] if r["launches"]}
        eng.profile_enable(0)
        calls = -(-int(fr.max()) // cf) + 1
        tail = {n: v for n, v in rows.items() if n.startswith(("chunk_", "stream_"))}
        return {"limiter": on, "calls": calls, "launches_per_call": sum(rows.values()) / calls, "delivery_launches": tail,
                "shaped_samples": shaped}

    per_leg = {name: [] for _, name in legs}
    firsts = {name: [] for _, name in legs}
    frames = None
    for rnd in range(args.rounds + 1):
        for on, name in legs:
            set_mode(on)
            t, first, frames, _ = stream()
            if rnd:                                      # round 0 captures the graphs
                per_leg[name].append(t)
                firsts[name].append(first)
    captures = eng.graph_stats[1]
    for on, name in legs:                                # ... and a steady server captures no more
        set_mode(on)
        stream()
    assert eng.graph_stats[1] == captures, (captures, eng.graph_stats)
    for on in (False, True):
        print(json.dumps({"tag": args.tag, "batch": B, **launches(on)}), flush=True)
    _, ms, Wn, D = eng.stream_limiter()
    eng.set_stream_gain("chunk")

    def p50(x):
        return float(np.median(np.asarray(x))) * 1e3

    out = {}
    for _, name in legs:
        rounds = per_leg[name]
        allt = [v for r in rounds for v in r]
        out[name] = {"p50_ms": p50(allt), "p10_ms": float(np.percentile(allt, 10)) * 1e3,
                     "p90_ms": float(np.percentile(allt, 90)) * 1e3, "round_p50_ms": [p50(r) for r in rounds],
                     "first_sample_p50_ms": p50(firsts[name]), "calls": len(allt)}
        print(json.dumps({"tag": args.tag, "leg": name, "voice": args.preset, "batch": B, "ids": T, "chunk_frames": cf,
                          "rate": eng.output_rate, "window_ms": ms, "W": Wn, "D": D,
                          "frames_min": int(frames.min()), "frames_max": int(frames.max()), **out[name]}), flush=True)
    aa = out["off"]["round_p50_ms"] + out["off (A/A)"]["round_p50_ms"]
    base = out["off"]["p50_ms"]
    verdict = {"tag": args.tag, "aa_p50_delta_ms": out["off (A/A)"]["p50_ms"] - base, "aa_round_p50_range_ms": max(aa) - min(aa),
               "on_minus_off_ms": out["on"]["p50_ms"] - base,
               "first_sample_on_minus_off_ms": out["on"]["first_sample_p50_ms"] - out["off"]["first_sample_p50_ms"],
               "graph_captures": captures}
    print(json.dumps(verdict), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
