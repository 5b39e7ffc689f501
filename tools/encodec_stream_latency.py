#!/usr/bin/env python3
"""Push latency of streaming EnCodec encode (Encodec.encode_stream) or decode (Encodec.decode_stream) on one GPU: EnCodec 24 kHz,
seeded synthetic weights, noise input / random tokens.

    python tools/encodec_stream_latency.py --batch 1 --frames 1 [--pushes 200 --warmup 20] [--direction decode]
    python tools/encodec_stream_latency.py --sweep [--out profiles/encodec_stream_latency.json]

Same method as tools/mimi_stream_latency.py: after the stream's own start-up hold (one push of WARMUP_FRAMES frames, not timed) and
`--warmup` untimed pushes, every push is timed on the host from `push` to a stream synchronisation (what a caller waiting for its
tokens sees).  Prints one JSON line per configuration: median / p99 push latency (ms), the real-time factor (audio seconds per
compute second, per stream and batch-wide), the per-kernel split of ONE further push (Encodec.profile_kernels: HIP-event time per
kernel name, launches) and, for scale, the one-shot time of a 10 s clip at the same batch size (`sig_to_toks` / `toks_to_sig`, median
of 5): what a caller without streaming pays for every new frame.  `--sweep` runs B = 1 / 8 / 64 with one-frame and 25-frame pushes
in both directions; `--out` also writes the lines as one JSON list."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiocodecs_amd import Encodec, checkpoint, prng  # noqa: E402
from audiocodecs_amd.config import ENCODEC_24KHZ  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def measure(codec, direction, B, F, pushes, warmup):
    cfg = codec.config
    hop, K = cfg.hop_length, codec.num_codebooks
    s = codec.encode_stream(B) if direction == "encode" else codec.decode_stream(B)
    W = s.WARMUP_FRAMES
    total = warmup + pushes + 1                      # + 1: the profiled push
    frames = W + total * F
    if direction == "encode":
        data = torch.from_numpy((prng.normal(11, "stream_latency", (B, frames * hop)) * 0.1).astype(np.float32)).cuda()
        piece = lambda a, n: data[:, a * hop:(a + n) * hop]      # noqa: E731
    else:
        data = torch.from_numpy(prng.randint(11, "stream_latency", (B, frames, K), cfg.codebook_size)).to(torch.int64).cuda()
        piece = lambda a, n: data[:, a:a + n]                    # noqa: E731
    first = s.push(piece(0, W))                      # the start-up hold, released as one push
    assert first.shape[1] == (W if direction == "encode" else W * hop)
    torch.cuda.synchronize()
    lat = []
    for i in range(warmup + pushes):
        t0 = time.perf_counter()
        out = s.push(piece(W + i * F, F))
        torch.cuda.synchronize()
        if i >= warmup:
            lat.append(time.perf_counter() - t0)
    assert out.shape[1] == (F if direction == "encode" else F * hop)
    stats = codec.profile_kernels(lambda: s.push(piece(W + (warmup + pushes) * F, F)))
    lat = np.array(lat) * 1e3
    med = float(np.median(lat))
    audio_ms = F * hop / cfg.sampling_rate * 1e3
    # the one-shot path on a 10 s clip at the same batch size
    n10 = 10 * cfg.sampling_rate // hop
    if direction == "encode":
        clip = torch.from_numpy((prng.normal(12, "stream_latency", (B, n10 * hop)) * 0.1).astype(np.float32)).cuda()
        one_shot = lambda: codec.sig_to_toks(clip)               # noqa: E731
    else:
        clip = torch.from_numpy(prng.randint(12, "stream_latency", (B, n10, K), cfg.codebook_size)).to(torch.int64).cuda()
        one_shot = lambda: codec.toks_to_sig(clip)               # noqa: E731
    one_shot()
    kern_ms = sum(ms for _, _, ms, _, _ in stats)
    return {"direction": direction, "batch": B, "frames_per_push": F, "pushes": pushes, "warmup": warmup,
            "median_ms": round(med, 3), "p99_ms": round(float(np.percentile(lat, 99)), 3), "audio_ms_per_push": audio_ms,
            "rtf_per_stream": round(audio_ms / med, 2), "rtf_batch": round(B * audio_ms / med, 2),
            "one_shot_10s_ms": round(timed(one_shot, 5), 3),
            "kernel_ms_one_push": round(kern_ms, 4), "launches_one_push": int(sum(n for _, n, _, _, _ in stats)),
            "kernels_one_push": [{"name": nm, "launches": n, "ms": round(ms, 4)} for nm, n, ms, _, _ in sorted(stats, key=lambda r: -r[2])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="frames (320 samples) per push")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default=None, choices=[None, "fp32", "fp32_exact"])
    ap.add_argument("--direction", default="encode", choices=["encode", "decode"])
    ap.add_argument("--sweep", action="store_true", help="B = 1 / 8 / 64 x 1 / 25 frames per push x both directions")
    ap.add_argument("--out", default=None, help="also write the result lines to this file as one JSON list")
    a = ap.parse_args()
    cfg = ENCODEC_24KHZ
    codec = Encodec(24000, num_codebooks=8, state_dict=checkpoint.synthetic_state_dict(cfg, seed=0), config=cfg, precision=a.precision).eval()
    runs = [(d, B, F) for d in ("encode", "decode") for B in (1, 8, 64) for F in (1, 25)] if a.sweep else [(a.direction, a.batch, a.frames)]
    rows = []
    for d, B, F in runs:
        rows.append(measure(codec, d, B, F, a.pushes, a.warmup))
        rows[-1]["precision"] = a.precision or "default"
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
