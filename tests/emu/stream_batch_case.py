"""The ragged three-utterance batch stream of tests/test_stream_batch_emu.py, shared with its child-process helper: the
inputs, and one drain of Engine.stream_batch. Run as a script it drains the stream once on the emulator build under the
fiber order EMU_ORDER names (the emulator reads the variable once per process) and prints one JSON line with a digest of
the int16 output."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from piper_amd import _lib as L, weights as W            # noqa: E402
from piper_amd.engine import Engine                      # noqa: E402

LENS = (6, 14, 23)
# three different triples; the length scales spread the frame counts so that the shortest utterance is finished several
# chunks of 4 frames before the longest
SCALES = np.array([[0.667, 0.5, 0.8], [0.3, 0.8, 0.5], [0.5, 1.0, 1.0]], np.float32)
# the multi-speaker tiny voice speaks about 3.5 times slower with its synthetic weights: its own rates, same raggedness
SCALES_MS = np.array([[0.667, 0.12, 0.8], [0.3, 0.18, 0.5], [0.5, 0.22, 1.0]], np.float32)
SIDS = (1, 3, 0)
CHUNK = 4


def inputs(cfg, seed=31):
    ids = [W.synthetic_phoneme_ids(T, 40 + i, id_max=cfg.n_vocab - 1) for i, T in enumerate(LENS)]
    rng = np.random.default_rng(seed)
    Tm = max(LENS)
    return (ids, rng.standard_normal((len(LENS), 2, Tm)).astype(np.float32),
            rng.standard_normal((len(LENS), cfg.inter, 48 * Tm + 64)).astype(np.float32))


def drain(eng, ids, nw, nz, sids=None, chunk_frames=CHUNK, want_audio=True, scales=SCALES):
    """Every chunk of the stream: ([per utterance: list of (float, int16) chunks, empty ones dropped], frames_done per call)."""
    per = [[] for _ in ids]
    done = []
    for item in eng.stream_batch(ids, scales, sids=sids, chunk_frames=chunk_frames, noise_w=nw, noise_z=nz,
                                 want_audio=want_audio):
        done.append(eng.stream_frames_done.copy())
        for b, (a, p) in enumerate(item):
            assert a is None or a.shape == p.shape
            if p.size:
                per[b].append((a, p))
    return per, done


def main():
    elib = L.bind(os.path.join(ROOT, "tests", "emu", "libpiper_hip_emu.so"))
    cfg = W.preset("tiny")
    w = W.synthetic_weights(cfg, 1234)
    ids, nw, nz = inputs(cfg)
    eng = Engine(blob=W.pack_blob(cfg, w), lib=elib)
    per, _ = drain(eng, ids, nw, nz)
    h = hashlib.sha256()
    for chunks in per:
        for _, p in chunks:
            h.update(np.ascontiguousarray(p).tobytes())
    print(json.dumps({"order": os.environ.get("EMU_ORDER", ""), "chunks": [len(c) for c in per],
                      "frames": [int(f) for f in eng.stream_frames], "pcm_sha256": h.hexdigest()}))
    eng.close()


if __name__ == "__main__":
    main()
