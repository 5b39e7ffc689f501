#!/usr/bin/env python3
"""Call latency of `stoi` against the reference's regime restated, on one GPU.

    python tools/stoi_latency.py [--calls 100 --host-calls 3 --warmup 3] [--out profiles/stoi_latency.jsonl]

One process; per shape (clips x seconds at 24 kHz, hypotheses P) in (64 x 10 s, 1), (64 x 10 s, 3), (1 x 10 s, 1) two forms run on the
SAME data on alternating calls (same clocks, same cache state) for as long as the slower form has calls left:
    fused    `stoi(hyp [P, B, T], ref, 24000)`: the library's resampler, then ac_stoi; nothing leaves the device but the scores
    host     downstream/metrics/stoi.py restated: the library's resampler to 16 kHz on the device (torchaudio is not installed), both
             signals moved to the host, then per hypothesis and clip, in a Python loop, the fp64 numpy statement of pystoi's algorithm
             (tests/stoi_ref.py: pystoi is not installed; its own numpy code does the same steps, each clip on its own)
Every call is timed on the host from the call to the scores being on the host.  One JSON line per shape: median / p99 (ms) of each form,
the largest absolute difference of the two results and the shader clock sampled while calls are queued (None where the platform
reports none).  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import stoi  # noqa: E402
from audiocodecs_amd.resample import resample  # noqa: E402
from latency_common import alternate, emit, median_p99, shader_mhz  # noqa: E402

SHAPES = ((64, 10, 1), (64, 10, 3), (1, 10, 1))
RATE = 24000


def host_regime(hyp, ref, R):
    r16 = resample(ref, RATE, 16000).cpu().numpy()
    out = []
    for p in range(hyp.shape[0]):
        h16 = resample(hyp[p], RATE, 16000).cpu().numpy()
        out.append([R.details(h, r)["score"] for h, r in zip(h16, r16)])
    return np.array(out)


def main():
    import stoi_ref as R

    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="timed calls of the fused form per shape")
    ap.add_argument("--host-calls", type=int, default=3, help="timed calls of the host form per shape (seconds each at 64 clips)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of the fused form (one of the host form)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for B, secs, P in SHAPES:
        T = secs * RATE
        ref = torch.from_numpy(np.stack([R.make_clip("gaps", 1000 * B + b, T) for b in range(B)])).cuda()
        g = torch.Generator().manual_seed(B + P)
        hyp = ref[None] + (0.01 * torch.randn(P, B, T, generator=g)).cuda()
        for _ in range(a.warmup):
            stoi(hyp, ref, RATE).cpu()
        host_regime(hyp, ref, R)
        forms = {"fused": lambda: stoi(hyp, ref, RATE).cpu(), "host": lambda: host_regime(hyp, ref, R)}
        lat, last = alternate(forms, {"fused": a.calls, "host": a.host_calls}, sync=False)      # (both forms end on the host)
        row = {"clips": B, "seconds": secs, "rate": RATE, "P": P, "frames": R.num_frames(secs * 16000), "calls": a.calls, "host_calls": a.host_calls, "warmup": a.warmup}
        for name, v in lat.items():
            row.update(median_p99(v, prefix=f"{name}_"))
        for _ in range(20):
            stoi(hyp, ref, RATE)
        row["shader_mhz"] = shader_mhz()
        torch.cuda.synchronize()
        row["largest_absolute_difference"] = float(np.abs(last["fused"].numpy().astype(np.float64) - last["host"]).max())
        emit(row, a.out)


if __name__ == "__main__":
    main()
