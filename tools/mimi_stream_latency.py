#!/usr/bin/env python3
"""Push latency of streaming Mimi encode (Mimi.encode_stream) on one GPU: full Mimi, seeded synthetic weights, noise input.

    python tools/mimi_stream_latency.py --batch 1 --frames 1 [--pushes 200 --warmup 20]

Every push is timed on the host from `push` to a stream synchronisation (what a caller waiting for its tokens sees).  Prints one
JSON line: median / p99 push latency (ms), the real-time factor (audio seconds per compute second, per stream and batch-wide) and
the configuration.  Launches per push come from a separate `rocprofv3 --kernel-trace --stats -- python tools/mimi_stream_latency.py
... --pushes N --warmup 0` run: dispatches in the stats divided by N."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiocodecs_amd import Mimi, checkpoint, prng  # noqa: E402
from audiocodecs_amd.config import MIMI_24KHZ  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="frames (1920 samples) per push")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default=None, choices=[None, "fp32", "fp32_exact"])
    a = ap.parse_args()
    cfg = MIMI_24KHZ
    codec = Mimi(24000, state_dict=checkpoint.synthetic_mimi_state_dict(cfg, seed=0), config=cfg, precision=a.precision).eval()
    n = a.frames * cfg.hop_length
    total = a.warmup + a.pushes
    sig = torch.from_numpy((prng.normal(11, "stream_latency", (a.batch, total * n)) * 0.1).astype(np.float32)).cuda()
    s = codec.encode_stream(a.batch)
    torch.cuda.synchronize()
    lat = []
    for i in range(total):
        t0 = time.perf_counter()
        toks = s.push(sig[:, i * n:(i + 1) * n])
        torch.cuda.synchronize()
        if i >= a.warmup:
            lat.append(time.perf_counter() - t0)
    assert toks.shape == (a.batch, a.frames, codec.num_codebooks)
    lat = np.array(lat) * 1e3
    audio_ms = a.frames * cfg.hop_length / cfg.sampling_rate * 1e3
    med = float(np.median(lat))
    print(json.dumps({"batch": a.batch, "frames_per_push": a.frames, "pushes": a.pushes, "precision": a.precision or "default",
                      "median_ms": round(med, 3), "p99_ms": round(float(np.percentile(lat, 99)), 3),
                      "audio_ms_per_push": audio_ms, "rtf_per_stream": round(audio_ms / med, 2),
                      "rtf_batch": round(a.batch * audio_ms / med, 2)}))


if __name__ == "__main__":
    main()
