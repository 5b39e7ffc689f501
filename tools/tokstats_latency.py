#!/usr/bin/env python3
"""Time of `CodebookUtil.append` against the reference's arithmetic as torch ops on the same GPU, and of one `resynthesis_report` against
the three `resynthesis_*` calls it replaces, on one GPU.

    python tools/tokstats_latency.py [--repeats 200 --ref-repeats 5 --report-repeats 10 --warmup 5] [--out profiles/tokstats_latency.jsonl]

One process, one JSON line per measurement.  Token shapes: 64 x 750 x 8 at C = 1024 (64 clips of 10 s of EnCodec at 8 codebooks) and
128 x 125 x 8 at C = 2048 (Mimi's).  The forms run on the SAME tokens on alternating repeats:
    append     `CodebookUtil.append(toks)`: one launch, nothing read back.  Timed with device events around the call (the kernel and the
               host's part of issuing it, whichever is longer) and with the host clock up to a synchronise.
    bincount   one `torch.bincount` of `toks + k C` on the device (it reads the largest id back to size its result).
    reference  downstream/metrics/codebook_util.py's arithmetic per clip and codebook: `unique(return_counts=True)` on the device, both
               results to the host, an indexed add into fp32 counts there.  Host clock (it ends on the host).
The report part runs the full-size EnCodec with seeded random weights on 64 clips of 10 s and the committed P.808 weights: one
`resynthesis_report` against `resynthesis_distances` + `resynthesis_stoi` + `resynthesis_dnsmos`, host clock up to a synchronise.
Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import CodebookUtil  # noqa: E402
from latency_common import emit, host_timed, median_p99  # noqa: E402

SHAPES = [("encodec", 64, 750, 8, 1024), ("mimi", 128, 125, 8, 2048)]


def reference_append(counts, toks):
    """What the reference does for a batch, clip by clip (its class takes B == 1 only)."""
    for b in range(toks.shape[0]):
        clip = toks[b:b + 1]
        for k in range(clip.shape[-1]):
            ids, n = clip[..., k].unique(return_counts=True)
            ids, n = ids.cpu(), n.cpu()
            counts[k][ids] += n


def stats(ms):
    return {**median_p99(ms, digits=4), "repeats": len(ms)}


def event_timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure_append(name, B, N, K, Cv, a):
    g = torch.Generator().manual_seed(B + N)
    toks = torch.randint(0, Cv, (B, N, K), generator=g).cuda()
    metric = CodebookUtil(K, Cv)
    offsets = (torch.arange(K, device="cuda") * Cv)[None, None, :]
    bincount = lambda: torch.bincount((toks + offsets).flatten(), minlength=K * Cv)
    ref_counts = [torch.zeros(Cv) for _ in range(K)]
    for _ in range(a.warmup):
        metric.append(toks)
        bincount()
    reference_append(ref_counts, toks)
    metric.clear()
    for c in ref_counts:
        c.zero_()
    ev, host, binc, ref = [], [], [], []
    for i in range(a.repeats):
        ev.append(event_timed(lambda: metric.append(toks)))
        host.append(host_timed(lambda: metric.append(toks)))
        binc.append(host_timed(bincount))
        if i < a.ref_repeats:
            ref.append(host_timed(lambda: reference_append(ref_counts, toks)))
    ours = metric.state.counts.cpu()
    exact = bool(torch.equal(ours, bincount().view(K, Cv).cpu() * (2 * a.repeats)))
    return {"what": "append", "shape": name, "B": B, "N": N, "K": K, "C": Cv, "append_events": stats(ev), "append_host": stats(host),
            "bincount_host": stats(binc), "reference_host": stats(ref), "counts_equal_bincount": exact}


def measure_report(a):
    from audiocodecs_amd import Encodec, checkpoint
    from audiocodecs_amd.config import ENCODEC_24KHZ as cfg
    from audiocodecs_amd.dnsmos import load_weights
    import dnsmos_ref as R

    weights = load_weights(os.path.join(ROOT, "tests", "golden", "dnsmos_p808.npz"))
    codec = Encodec(24000, num_codebooks=8, state_dict=checkpoint.synthetic_state_dict(cfg, seed=0)).eval()
    B, T = 64, 240000
    sig = torch.from_numpy(np.stack([R.make_signal(R.KINDS[b % 3], T, seed=b) for b in range(B)])).cuda()
    metric = CodebookUtil(8, cfg.codebook_size)
    one = lambda: codec.resynthesis_report(sig, dnsmos_weights=weights, codebook_util=metric)
    three = lambda: (codec.resynthesis_distances(sig), codec.resynthesis_stoi(sig), codec.resynthesis_dnsmos(sig, weights))
    for _ in range(max(1, a.warmup // 2)):
        one()
        three()
    t1, t3 = [], []
    for _ in range(a.report_repeats):
        t1.append(host_timed(one))
        t3.append(host_timed(three))
    r = one()
    s = three()
    same = all(bool(torch.equal(x, y)) for x, y in zip((r["stft"], r["mel"], r["stoi"], r["dnsmos"]), (*s[0], s[1], s[2])))
    return {"what": "report", "codec": "encodec_24khz", "B": B, "seconds": 10, "report_host": stats(t1), "three_calls_host": stats(t3), "results_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--ref-repeats", type=int, default=5)
    ap.add_argument("--report-repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-report", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    jobs = [lambda shape=shape: measure_append(*shape, a) for shape in SHAPES] + ([] if a.no_report else [lambda: measure_report(a)])
    for job in jobs:
        emit(job(), a.out)


if __name__ == "__main__":
    main()
