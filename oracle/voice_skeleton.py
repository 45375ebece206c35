"""TEST INFRASTRUCTURE -- full-size exported voices without the reference. A .onnx written by the reference's export path
(oracle/make_voice.py) is ~1 MB of graph around the seeded synthetic weights: strip() empties the payload of every
initialiser that is a seeded weight, or the flow's folded weight norm of one, and names its source in the tensor's
doc_string; fill() puts the payloads back from W.synthetic_weights and returns the exported file byte for byte
(tests/golden/full/manifest.json holds its SHA-256). The stripped files are the fixtures under tests/golden/full/:

    python oracle/voice_skeleton.py strip <exported .onnx> <preset> <out .onnx.gz>
"""
import gzip
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import onnx_mutate as M  # noqa: E402
from piper_amd import weights as W  # noqa: E402

FULL = os.path.join(ROOT, "tests", "golden", "full")
_RAW, _DOC = 9, 12                       # TensorProto raw_data / doc_string


def _folded(w):
    """The flow's weight norm as the export folds it (weight_v = w, weight_g = |w| per output channel)."""
    import torch
    v = torch.from_numpy(np.ascontiguousarray(w, np.float32))
    g = v.flatten(1).norm(dim=1).view(-1, 1, 1)
    return (torch.div(v, torch.norm_except_dim(v, 2, 0)) * g).numpy()


def _payloads(preset):
    w = W.synthetic_weights(W.preset(preset), 1234)
    return {f"w:{k}": np.ascontiguousarray(v, np.float32).tobytes() for k, v in w.items()}, w


def _map_inits(data, fn):
    """Apply fn(tensor fields) -> fields to every initialiser; every other byte of the model is kept as it is."""
    model = M.parse(data)
    for gi, (f, wt, graph) in enumerate(model):
        if f == 7:
            g = [(gf, gwt, M.serialize(fn(M.parse(v))) if gf == 5 else v) for gf, gwt, v in M.parse(graph)]
            model[gi] = (f, wt, M.serialize(g))
    return M.serialize(model)


def strip(data, preset):
    plain, w = _payloads(preset)
    by_bytes = {v: k for k, v in plain.items()}
    for k, v in w.items():
        if v.ndim == 3:
            by_bytes.setdefault(_folded(v).tobytes(), f"wn:{k}")

    def fn(t):
        raw = M._get(t, _RAW)
        src = by_bytes.get(raw[0]) if raw and len(raw[0]) >= 1024 else None
        if src is None:
            return t
        return [(f, wt, b"" if f == _RAW else v) for f, wt, v in t] + [(_DOC, 2, src.encode())]
    return _map_inits(data, fn)


def fill(name, out_dir):
    """Writes the full-size voice `name` of tests/golden/full/ (a .onnx + its .onnx.json, or a streaming directory) under
    out_dir and returns its path."""
    man = json.load(open(os.path.join(FULL, "manifest.json")))
    cache = {}
    for rel, e in man.items():
        if rel != name and not rel.startswith(name + "/") and rel != name + ".json":
            continue
        dst = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        src = os.path.join(FULL, rel)
        if not rel.endswith(".onnx"):
            with open(src, "rb") as fi, open(dst, "wb") as fo:
                fo.write(fi.read())
            continue
        if e["preset"] not in cache:
            cache[e["preset"]] = _payloads(e["preset"])
        plain, w = cache[e["preset"]]

        def fn(t):
            doc = M._get(t, _DOC)
            if not doc or not doc[0].startswith((b"w:", b"wn:")):
                return t
            key = doc[0].decode()
            raw = plain[key] if key.startswith("w:") else _folded(w[key[3:]]).tobytes()
            return [(f, wt, raw if f == _RAW else v) for f, wt, v in t if f != _DOC]
        data = _map_inits(gzip.decompress(open(src + ".gz", "rb").read()), fn)
        if hashlib.sha256(data).hexdigest() != e["sha256"]:
            raise RuntimeError(f"{rel}: the refilled voice is not the exported file")
        with open(dst, "wb") as f:
            f.write(data)
    return os.path.join(out_dir, name)


if __name__ == "__main__" and sys.argv[1] == "strip":
    src, preset, out = sys.argv[2:5]
    data = open(src, "rb").read()
    with open(out, "wb") as f:
        f.write(gzip.compress(strip(data, preset), 9, mtime=0))
    print(out, preset, hashlib.sha256(data).hexdigest())
