#!/usr/bin/env python
"""What a listener who arrives in the middle of a batch stream waits for, with the stream pool and without it.

In ONE process, per voice (high, medium), a pool of 64 slots, 128 ids per utterance, noise drawn by the engine, chunks of
45 frames, every shape warmed first, then `--reps` repetitions with the legs alternating, host clock around work that ends
in a synchronisation, p50:

  (a) join      63 residents are two chunks into their stream; pe_stream_pool_join of ONE newcomer .. return of the
                pe_stream_pool_next that delivers its first 45 frames
      baseline  what the engine could do for that request before the pool: 63 residents two chunks into a lock-step stream
                (pe_stream_begin_batch); drain them (pe_stream_next_batch until finished), then pe_stream_begin_batch of the
                newcomer alone + its first pe_stream_next_batch
  (b) period    one pe_stream_pool_next with the 63 residents undisturbed, against the join of (a) split into its
                pe_stream_pool_join and the next call, now of 64 listeners: how much later the residents' chunk arrives
  (c) two live  one pe_stream_pool_next with 2 of the 64 slots occupied, against one pe_stream_next_batch of a 2-utterance
                lock-step stream: what running the window stage over empty slots costs

Prints one JSON line per voice and the markdown rows of profiles/stream_join.md.

    python scripts/stream_join_latency.py [--reps 20] [--voices high medium]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from piper_amd import _lib as L, weights as W            # noqa: E402
from piper_amd.engine import Engine                      # noqa: E402

SCALES = (0.667, 1.0, 0.8)
CHUNK, SLOTS, MAX_FRAMES = 45, 64, 512


class Case:
    def __init__(self, voice, ids_per=128):
        cfg = W.preset(voice)
        self.eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
        self.lib, self.h = self.eng._lib, self.eng._h
        self.id_lists = [W.synthetic_phoneme_ids(ids_per, 60 + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(SLOTS)]
        self.p64, self.pf, self.p32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self.sc = np.ascontiguousarray(np.tile(np.asarray(SCALES, np.float32), (SLOTS, 1)))
        self.packed = {}
        self.slot_of, self.frames = np.zeros(SLOTS, np.int32), np.zeros(SLOTS, np.int32)
        halo = C.c_int32()
        self.ok(self.lib.pe_stream_pool_open(self.h, SLOTS, MAX_FRAMES, C.byref(halo)))

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.lib.pe_last_error().decode())

    def pack(self, lo, hi):
        if (lo, hi) not in self.packed:
            self.packed[lo, hi] = Engine._pack(self.id_lists[lo:hi])
        return self.packed[lo, hi]

    # ---- the pool
    def join(self, lo, hi):
        ids, offs = self.pack(lo, hi)
        self.ok(self.lib.pe_stream_pool_join(self.h, ids.ctypes.data_as(self.p64), offs.ctypes.data_as(self.p64), hi - lo,
                                             self.sc.ctypes.data_as(self.pf), None, None, self.slot_of.ctypes.data_as(self.p32),
                                             self.frames.ctypes.data_as(self.p32)))

    def next(self):
        ch = L.PeStreamChunk()
        self.ok(self.lib.pe_stream_pool_next(self.h, CHUNK, None, 0, C.byref(ch)))
        return int(ch.sample_offsets[SLOTS])

    def clear(self):
        live = np.zeros(SLOTS, np.int32)
        n = C.c_int32()
        self.ok(self.lib.pe_stream_pool_state(self.h, C.byref(n), None, None, live.ctypes.data_as(self.p32)))
        for s in np.flatnonzero(live):
            self.ok(self.lib.pe_stream_pool_leave(self.h, int(s)))

    # ---- the lock-step stream
    def begin(self, lo, hi):
        ids, offs = self.pack(lo, hi)
        halo = C.c_int32()
        self.ok(self.lib.pe_stream_begin_batch(self.h, ids.ctypes.data_as(self.p64), offs.ctypes.data_as(self.p64), hi - lo,
                                               self.sc.ctypes.data_as(self.pf), None, None, self.frames.ctypes.data_as(self.p32),
                                               C.byref(halo)))

    def next_batch(self, B):
        ch = L.PeStreamChunk()
        self.ok(self.lib.pe_stream_next_batch(self.h, CHUNK, 0, C.byref(ch)))
        return int(ch.sample_offsets[B])

    # ---- the legs
    def leg_pool(self):
        """-> (join + first chunk, join alone, the next call of 64, an undisturbed call of 63) in seconds"""
        self.clear()
        self.join(0, 63)
        self.next()
        t0 = time.perf_counter()
        self.next()                                       # the residents' second chunk, undisturbed
        t1 = time.perf_counter()
        self.join(63, 64)
        t2 = time.perf_counter()
        n = self.next()
        t3 = time.perf_counter()
        assert n == SLOTS * CHUNK * self.eng.hop
        return t3 - t1, t2 - t1, t3 - t2, t1 - t0

    def leg_baseline(self):
        self.begin(0, 63)
        self.next_batch(63)
        self.next_batch(63)
        t0 = time.perf_counter()
        while self.next_batch(63):
            pass
        self.begin(63, 64)
        n = self.next_batch(1)
        t1 = time.perf_counter()
        assert n == CHUNK * self.eng.hop
        return t1 - t0

    def leg_two_live(self, calls=4):
        self.clear()
        self.join(0, 2)
        self.next()
        t0 = time.perf_counter()
        for _ in range(calls):
            assert self.next() == 2 * CHUNK * self.eng.hop
        t1 = time.perf_counter()
        self.clear()
        self.begin(0, 2)
        self.next_batch(2)
        t2 = time.perf_counter()
        for _ in range(calls):
            assert self.next_batch(2) == 2 * CHUNK * self.eng.hop
        t3 = time.perf_counter()
        return (t1 - t0) / calls, (t3 - t2) / calls


def p50(v):
    return float(np.median(np.asarray(v)))


def measure(voice, reps):
    c = Case(voice)
    for _ in range(3):                        # every shape: graphs captured, workspaces at their final size
        c.leg_pool()
        c.leg_baseline()
        c.leg_two_live()
    captures0 = c.eng.graph_stats[1]
    t = dict(join_first=[], join=[], next64=[], next63=[], base=[], pool2=[], lock2=[])
    for _ in range(reps):
        a, b, d, e = c.leg_pool()
        t["join_first"].append(a), t["join"].append(b), t["next64"].append(d), t["next63"].append(e)
        t["base"].append(c.leg_baseline())
        p, q = c.leg_two_live()
        t["pool2"].append(p), t["lock2"].append(q)
    # (the engine draws the duration noise, so a repetition's longest utterance may land in a frame bucket no warm-up call
    # visited and capture one more graph: reported, and the median does not move for it)
    late_captures = c.eng.graph_stats[1] - captures0
    ms = {k: 1e3 * p50(v) for k, v in t.items()}
    row = {"voice": voice, "reps": reps, "slots": SLOTS, "chunk_frames": CHUNK,
           "join_to_first_chunk_ms": ms["join_first"], "baseline_drain_then_begin_ms": ms["base"],
           "ratio": ms["base"] / ms["join_first"], "join_alone_ms": ms["join"], "next_64_after_join_ms": ms["next64"],
           "undisturbed_next_63_ms": ms["next63"], "residents_delay_ms": ms["join_first"] - ms["next63"],
           "next_2_live_of_64_ms": ms["pool2"], "next_batch_2_ms": ms["lock2"], "graphs_captured_while_timing": late_captures}
    c.ok(c.lib.pe_stream_pool_close(c.h))
    c.eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--voices", nargs="+", default=["high", "medium"])
    a = ap.parse_args()
    rows = []
    for v in a.voices:
        rows.append(measure(v, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    print("\n| voice | (a) join .. newcomer's first chunk | drain the residents, then begin | ratio | (b) undisturbed chunk of 63 | "
          "join alone | chunk of 64 after it | residents' chunk arrives later by | (c) chunk, 2 live of 64 slots | chunk, lock-step B=2 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['voice']} | {r['join_to_first_chunk_ms']:.2f} ms | {r['baseline_drain_then_begin_ms']:.2f} ms | "
              f"{r['ratio']:.1f}x | {r['undisturbed_next_63_ms']:.2f} ms | {r['join_alone_ms']:.2f} ms | "
              f"{r['next_64_after_join_ms']:.2f} ms | {r['residents_delay_ms']:.2f} ms | {r['next_2_live_of_64_ms']:.2f} ms | "
              f"{r['next_batch_2_ms']:.2f} ms |")


if __name__ == "__main__":
    main()
