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
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import stoi  # noqa: E402
from audiocodecs_amd.resample import resample  # noqa: E402

SHAPES = ((64, 10, 1), (64, 10, 3), (1, 10, 1))
RATE = 24000


def host_regime(hyp, ref, R):
    r16 = resample(ref, RATE, 16000).cpu().numpy()
    out = []
    for p in range(hyp.shape[0]):
        h16 = resample(hyp[p], RATE, 16000).cpu().numpy()
        out.append([R.details(h, r)["score"] for h, r in zip(h16, r16)])
    return np.array(out)


def shader_mhz():
    try:
        return round(torch.cuda.clock_rate(), 0)
    except Exception:
        pass
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", str(torch.cuda.current_device())], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level:.*?\((\d+)Mhz\)", txt)
        return float(m.group(1)) if m else None
    except Exception:
        return None


def main():
    import stoi_ref as R

    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="timed calls of the fused form per shape")
    ap.add_argument("--host-calls", type=int, default=3, help="timed calls of the host form per shape (seconds each at 64 clips)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of the fused form (one of the host form)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []
    for B, secs, P in SHAPES:
        T = secs * RATE
        ref = torch.from_numpy(np.stack([R.make_clip("gaps", 1000 * B + b, T) for b in range(B)])).cuda()
        g = torch.Generator().manual_seed(B + P)
        hyp = ref[None] + (0.01 * torch.randn(P, B, T, generator=g)).cuda()
        for _ in range(a.warmup):
            stoi(hyp, ref, RATE).cpu()
        host_regime(hyp, ref, R)
        lat = {"fused": [], "host": []}
        for i in range(max(a.calls, a.host_calls)):
            if i < a.calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fused = stoi(hyp, ref, RATE).cpu()
                lat["fused"].append((time.perf_counter() - t0) * 1e3)
            if i < a.host_calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = host_regime(hyp, ref, R)
                lat["host"].append((time.perf_counter() - t0) * 1e3)
        row = {"clips": B, "seconds": secs, "rate": RATE, "P": P, "frames": R.num_frames(secs * 16000), "calls": a.calls, "host_calls": a.host_calls, "warmup": a.warmup}
        for name, v in lat.items():
            row[f"{name}_median_ms"] = round(float(np.median(v)), 3)
            row[f"{name}_p99_ms"] = round(float(np.percentile(v, 99)), 3)
        for _ in range(20):
            stoi(hyp, ref, RATE)
        row["shader_mhz"] = shader_mhz()
        torch.cuda.synchronize()
        row["largest_absolute_difference"] = float(np.abs(fused.numpy().astype(np.float64) - host).max())
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
