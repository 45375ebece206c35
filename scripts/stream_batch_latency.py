#!/usr/bin/env python
"""Time to the first chunk of a batch stream against what the same listeners get without it.

In ONE process, per voice (medium, high) and batch size (8, 64), 128 ids per utterance, noise drawn by the engine, every
shape warmed first, then `--reps` repetitions with the legs alternating, host clock around work that ends in a
synchronisation, p50:

  first     pe_stream_begin_batch .. return of the first pe_stream_next_batch (45 frames)
  whole     the whole pe_synthesize_batch call on the same inputs
  serial    B one-utterance pe_stream_begin + first pe_stream_next back to back: the LAST listener's wait
  drain     pe_stream_begin_batch + every pe_stream_next_batch until the batch is finished (samples/s next to `whole`'s)

Prints one JSON line per configuration and a markdown table (profiles/stream_batch.md). `--trace-only VOICE B` runs one
warmed batch stream and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times.

    python scripts/stream_batch_latency.py [--reps 50] [--voices medium high] [--batches 8 64]
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
CHUNK = 45


class Case:
    def __init__(self, voice, B, ids_per=128):
        cfg = W.preset(voice)
        self.eng = Engine(blob=W.pack_blob(cfg, W.synthetic_weights(cfg, 1234)), device=0)
        self.lib, self.h, self.B = self.eng._lib, self.eng._h, B
        id_lists = [W.synthetic_phoneme_ids(ids_per, 60 + i, id_max=min(cfg.n_vocab - 1, 129)) for i in range(B)]
        self.ids, self.offs = Engine._pack(id_lists)
        self.one = [np.ascontiguousarray(x, np.int64) for x in id_lists]
        self.sc1 = (C.c_float * 3)(*SCALES)
        self.scB = np.ascontiguousarray(np.tile(np.asarray(SCALES, np.float32), (B, 1)))
        self.frames = np.zeros(B, np.int32)
        self.p64, self.pf, self.p32 = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def ok(self, rc):
        if rc:
            raise RuntimeError(self.lib.pe_last_error().decode())

    def begin(self):
        halo = C.c_int32()
        self.ok(self.lib.pe_stream_begin_batch(self.h, self.ids.ctypes.data_as(self.p64), self.offs.ctypes.data_as(self.p64),
                                               self.B, self.scB.ctypes.data_as(self.pf), None, None,
                                               self.frames.ctypes.data_as(self.p32), C.byref(halo)))

    def next(self, want_audio=0):
        ch = L.PeStreamChunk()
        self.ok(self.lib.pe_stream_next_batch(self.h, CHUNK, want_audio, C.byref(ch)))
        return int(ch.sample_offsets[self.B])

    def first(self):
        t0 = time.perf_counter()
        self.begin()
        self.next()
        return time.perf_counter() - t0

    def drain(self):
        t0 = time.perf_counter()
        self.begin()
        total = 0
        while True:
            n = self.next()
            if n == 0:
                break
            total += n
        return time.perf_counter() - t0, total

    def whole(self):
        res = L.PeResult()
        t0 = time.perf_counter()
        self.ok(self.lib.pe_synthesize_batch(self.h, self.ids.ctypes.data_as(self.p64), self.offs.ctypes.data_as(self.p64),
                                             self.B, self.sc1, None, None, C.byref(res)))
        dt = time.perf_counter() - t0
        return dt, int(res.sample_offsets[self.B])

    def serial(self):
        fr, halo = C.c_int32(), C.c_int32()
        a, p, n = self.pf(), C.POINTER(C.c_int16)(), C.c_int64()
        t0 = time.perf_counter()
        for x in self.one:
            self.ok(self.lib.pe_stream_begin(self.h, x.ctypes.data_as(self.p64), x.size, self.sc1, -1, None, C.byref(fr),
                                             C.byref(halo)))
            self.ok(self.lib.pe_stream_next(self.h, CHUNK, C.byref(a), C.byref(p), C.byref(n)))
        return time.perf_counter() - t0


def p50(v):
    return float(np.median(np.asarray(v)))


def measure(voice, B, reps, drain_reps):
    c = Case(voice, B)
    for _ in range(3):                        # every shape: graphs captured, workspaces at their final size
        c.drain()
        c.whole()
        c.serial()
    t = dict(first=[], whole=[], serial=[], drain=[])
    s_whole = s_drain = 0
    for r in range(reps):
        t["first"].append(c.first())
        dt, s_whole = c.whole()
        t["whole"].append(dt)
        t["serial"].append(c.serial())
        if r < drain_reps:
            dt, s_drain = c.drain()
            t["drain"].append(dt)
    row = {"voice": voice, "batch": B, "reps": reps, "frames_min": int(c.frames.min()), "frames_max": int(c.frames.max()),
           "first_chunk_ms": 1e3 * p50(t["first"]), "whole_call_ms": 1e3 * p50(t["whole"]),
           "serial_first_chunks_ms": 1e3 * p50(t["serial"]), "drain_ms": 1e3 * p50(t["drain"]),
           "drain_samples_per_s": s_drain / p50(t["drain"]), "whole_samples_per_s": s_whole / p50(t["whole"])}
    c.eng.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--drain-reps", type=int, default=20)
    ap.add_argument("--voices", nargs="+", default=["medium", "high"])
    ap.add_argument("--batches", nargs="+", type=int, default=[8, 64])
    ap.add_argument("--trace-only", nargs=2, metavar=("VOICE", "BATCH"))
    a = ap.parse_args()
    if a.trace_only:
        c = Case(a.trace_only[0], int(a.trace_only[1]))
        for _ in range(3):
            c.drain()
        c.eng.close()
        return
    rows = []
    for v in a.voices:
        for B in a.batches:
            rows.append(measure(v, B, a.reps, min(a.reps, a.drain_reps)))
            print(json.dumps(rows[-1]), flush=True)
    print("\n| voice | B | frames | first chunk, batch stream | whole call | B x one-utterance first chunk | drained stream | whole call |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['voice']} | {r['batch']} | {r['frames_min']}..{r['frames_max']} | {r['first_chunk_ms']:.2f} ms | "
              f"{r['whole_call_ms']:.2f} ms | {r['serial_first_chunks_ms']:.2f} ms | {r['drain_samples_per_s'] / 1e6:.2f} Msamples/s | "
              f"{r['whole_samples_per_s'] / 1e6:.2f} Msamples/s |")


if __name__ == "__main__":
    main()
