#!/usr/bin/env python3
"""Call latency of `knn_match` against a torch restatement of the reference's k-NN helper, on one GPU.

    python tools/knn_match_latency.py [--calls 100 --warmup 5] [--out profiles/knn_match_latency.jsonl]

One process; per shape (Q query rows, M set rows) in (400, 2400), (400, 24000), (25600, 24000) at H = 512, k = 4 three forms run on the
SAME data on alternating calls (same clocks, same cache state):
    packed      `KnnIndex.match` on an index packed once, outside the timed call
    per_call    `knn_match(feats, set)`: packs the set inside every call
    torch       the reference helper's arithmetic (downstream/test_vc.py:345-382, num_splits = 1) followed by its `.mean(dim=-2)`, restated
                in torch on the same device: |q|^2 + |t|^2 - cdist^2, top-k of the [Q, M] matrix, gather, mean
Every call is timed on the host from the call to a stream synchronisation.  One JSON line per shape: median / p99 (ms) of each form, the
split count the library chose, the agreement of the two results (rows whose neighbour sets are equal) and the shader clock sampled while
matches are queued (None where the platform reports none).  The timed calls per form are `--calls` or as many as keep the fastest form
busy for `--window` seconds, whichever is more.  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiocodecs_amd import KnnIndex, knn_match  # noqa: E402
from audiocodecs_amd.knn import auto_splits  # noqa: E402
from latency_common import alternate_for, emit, median_p99, shader_mhz  # noqa: E402

SHAPES = ((400, 2400), (400, 24000), (25600, 24000))
H, TOPK = 512, 4


def torch_helper(q, t, topk):
    qn, tn = (q ** 2).sum(dim=-1), (t ** 2).sum(dim=-1)
    dot = (qn[:, None] + tn[None] - torch.cdist(q[None], t[None])[0] ** 2) / 2
    dist = 1 - dot * (qn[:, None] * tn[None]).rsqrt()
    idx = dist.topk(k=min(topk, t.shape[0]), largest=False, dim=-1).indices
    return t[idx].mean(dim=-2), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="least number of timed calls per form and shape")
    ap.add_argument("--window", type=float, default=1.0, help="least timed seconds of the fastest form per shape")
    ap.add_argument("--max-calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for Q, M in SHAPES:
        g = torch.Generator().manual_seed(Q + M)
        centres = torch.randn(200, H, generator=g)                # feature-like rows: clusters of directions with noise and a spread of norms
        def rows(n):
            return ((centres[torch.randint(0, 200, (n,), generator=g)] + 0.3 * torch.randn(n, H, generator=g)) * torch.exp(torch.randn(n, 1, generator=g))).cuda()
        q, t = rows(Q), rows(M)
        index = KnnIndex(t)
        forms = {
            "packed": lambda: index.match(q, topk=TOPK),
            "per_call": lambda: knn_match(q, t, topk=TOPK),
            "torch": lambda: torch_helper(q, t, TOPK)[0],
        }
        lat, last, calls = alternate_for(forms, a.calls, a.window, a.max_calls, a.warmup)
        assert all(out.shape == (Q, H) for out in last.values())
        row = {"Q": Q, "M": M, "H": H, "topk": TOPK, "num_splits": auto_splits(Q, M, H), "calls": calls, "warmup": a.warmup}
        for name, v in lat.items():
            row.update(median_p99(v, prefix=f"{name}_"))
        for _ in range(20):
            index.match(q, topk=TOPK)
        row["shader_mhz"] = shader_mhz()
        torch.cuda.synchronize()
        _, idx, _ = index.match(q, topk=TOPK, return_indices=True)
        tidx = torch_helper(q, t, TOPK)[1]
        row["rows_with_the_same_neighbour_set"] = int((idx.sort(dim=-1).values == tidx.sort(dim=-1).values).all(dim=-1).sum())
        emit(row, a.out)


if __name__ == "__main__":
    main()
