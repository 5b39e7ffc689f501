#!/usr/bin/env python3
"""Generate tests/golden/knn_golden.npz from the reference's own k-NN helper.

    python tools/make_knn_golden.py

The fixture pins tests/knn_ref.py (the project's fp64 statement of cosine k-NN matching and its checker) to the reference's code:
the two functions `_cosine_distance` and `knn` are taken out of /root/reference/downstream/test_vc.py AT GENERATION TIME -- the module
itself cannot be imported (speechbrain is not installed) -- compiled from the file's syntax tree and run in fp64, where the
cancellation of their `|q|^2 + |t|^2 - cdist^2` form is harmless.  None of their text is stored: the file holds data only -- per case the
inputs, the neighbours the helper gathered, the indices of those neighbours in the set (recovered by comparing rows) and their mean.

Inputs are seeded Gaussian rows rounded to small integers (int8): exact in every number format on the way, and the file stays small.
Cases (Q, M, H, k): (64, 300, 32, 4); (33, 5, 128, 8), a set smaller than topk; (48, 97, 512, 1).
"""
import ast
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = "/root/reference/downstream/test_vc.py"
CASES = ((64, 300, 32, 4), (33, 5, 128, 8), (48, 97, 512, 1))


def reference_functions():
    src = open(SOURCE).read()
    wanted = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in ("_cosine_distance", "knn")]
    assert sorted(n.name for n in wanted) == ["_cosine_distance", "knn"], "the reference helper moved"
    ns = {"torch": torch}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), SOURCE, "exec"), ns)
    return ns["knn"]


def main():
    knn = reference_functions()
    out, meta = {}, {"source": "downstream/test_vc.py: _cosine_distance, knn (run in fp64)", "torch": torch.__version__, "cases": []}
    for c, (Q, M, H, k) in enumerate(CASES):
        rng = np.random.default_rng(1000 + c)
        q = np.clip(np.rint(rng.standard_normal((Q, H)) * 24), -127, 127).astype(np.int8)
        t = np.clip(np.rint(rng.standard_normal((M, H)) * 24), -127, 127).astype(np.int8)
        nb = knn(torch.from_numpy(q.astype(np.float64)), torch.from_numpy(t.astype(np.float64)), topk=k, num_splits=1).numpy()
        kk = min(k, M)
        assert nb.shape == (Q, kk, H) and nb.dtype == np.float64
        idx = np.full((Q, kk), -1, dtype=np.int16)
        for i in range(Q):
            for j in range(kk):
                hit = np.nonzero((t.astype(np.float64) == nb[i, j]).all(axis=1))[0]
                assert len(hit) == 1, "a neighbour must be exactly one row of the set"
                idx[i, j] = hit[0]
        assert (nb == np.rint(nb)).all()
        out[f"c{c}_q"], out[f"c{c}_t"] = q, t
        out[f"c{c}_neighbours"] = nb.astype(np.int8)
        out[f"c{c}_idx"] = idx
        out[f"c{c}_mean"] = nb.mean(axis=-2)
        meta["cases"].append({"Q": Q, "M": M, "H": H, "topk": k})
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "knn_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
