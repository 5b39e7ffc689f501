#!/usr/bin/env python3
"""Push latency of streaming Mimi encode (Mimi.encode_stream) or decode (Mimi.decode_stream) on one GPU: full Mimi, seeded synthetic
weights, noise input / random tokens.

    python tools/mimi_stream_latency.py --batch 1 --frames 1 [--pushes 200 --warmup 20] [--direction decode [--linear-route ab]]

`--linear-route` (decode only) forces the route of a push's linear layers (ac_debug_set "mstream_skinny"): `tap` = the tap-GEMM,
`skinny` = mstream_linear_kernel, `auto` = the library's rule, `ab` = tap and skinny on alternate pushes of ONE stream in ONE process
(the A/B the auto threshold comes from: same clocks, same cache state; `--pushes` counts the pushes of each route).

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
    ap.add_argument("--direction", default="encode", choices=["encode", "decode"])
    ap.add_argument("--linear-route", default="auto", choices=["auto", "tap", "skinny", "ab"], help="decode only")
    a = ap.parse_args()
    if a.direction == "decode":
        return decode(a)
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


def decode(a):
    from audiocodecs_amd import _native

    cfg = MIMI_24KHZ
    codec = Mimi(24000, state_dict=checkpoint.synthetic_mimi_state_dict(cfg, seed=0), config=cfg, precision=a.precision).eval()
    ab = a.linear_route == "ab"
    total = a.warmup + a.pushes * (2 if ab else 1)
    toks = torch.from_numpy(prng.randint(11, "stream_latency", (a.batch, total * a.frames, codec.num_codebooks), cfg.codebook_size)).to(torch.int64).cuda()
    s = codec.decode_stream(a.batch)
    routes = {"auto": -1, "tap": 0, "skinny": 1}
    if not ab:
        _native.debug_set(codec, "mstream_skinny", routes[a.linear_route])
    torch.cuda.synchronize()
    lat = {0: [], 1: []}
    for i in range(total):
        if ab:
            _native.debug_set(codec, "mstream_skinny", i & 1)
        t0 = time.perf_counter()
        sig = s.push(toks[:, i * a.frames:(i + 1) * a.frames])
        torch.cuda.synchronize()
        if i >= a.warmup:
            lat[i & 1 if ab else 0].append(time.perf_counter() - t0)
    assert sig.shape == (a.batch, a.frames * cfg.hop_length)
    audio_ms = a.frames * cfg.hop_length / cfg.sampling_rate * 1e3
    out = {"direction": "decode", "batch": a.batch, "frames_per_push": a.frames, "rows_per_launch": a.batch * a.frames * cfg.resample_stride,
           "pushes": a.pushes, "precision": a.precision or "default", "linear_route": a.linear_route, "audio_ms_per_push": audio_ms}
    for key, name in ((0, "tap" if ab else None), (1, "skinny" if ab else None)):
        if not lat[key]:
            continue
        v = np.array(lat[key]) * 1e3
        pre = f"{name}_" if name else ""
        med = float(np.median(v))
        out.update({f"{pre}median_ms": round(med, 3), f"{pre}p99_ms": round(float(np.percentile(v, 99)), 3),
                    f"{pre}rtf_per_stream": round(audio_ms / med, 2), f"{pre}rtf_batch": round(a.batch * audio_ms / med, 2)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
