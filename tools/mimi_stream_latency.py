#!/usr/bin/env python3
"""Push latency of streaming Mimi encode (Mimi.encode_stream) or decode (Mimi.decode_stream) on one GPU: full Mimi, seeded synthetic
weights, noise input / random tokens.

    python tools/mimi_stream_latency.py --batch 1 --frames 1 [--pushes 200 --warmup 20] [--direction decode [--linear-route ab]]
    python tools/mimi_stream_latency.py --sessions --out profiles/mimi_sessions_latency.json

`--linear-route` (decode only) forces the route of a push's linear layers (ac_debug_set "mstream_skinny"): `tap` = the tap-GEMM,
`skinny` = mstream_linear_kernel, `auto` = the library's rule, `ab` = tap and skinny on alternate pushes of ONE stream in ONE process
(the A/B the auto threshold comes from: same clocks, same cache state; `--pushes` counts the pushes of each route).

`--sessions` measures session pools (Mimi.encode_sessions / decode_sessions): a pool of capacity 64 with
n = 1 / 8 / 64 listed slots against the lockstep stream of batch n, one-frame pushes, both directions, the two timed on alternating
pushes of ONE process (same clocks, same cache state), and the mixed tick: one freshly opened slot beside n - 1 slots that are more
than 125 frames (a full window of 250 positions) old.  One JSON line per (direction, n); `--out` also writes them as one JSON list.

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


def measure_sessions(codec, direction, n, pushes, warmup, capacity=64, old_frames=130):
    cfg = codec.config
    hop, K = cfg.hop_length, codec.num_codebooks
    enc = direction == "encode"
    pool = codec.encode_sessions(capacity) if enc else codec.decode_sessions(capacity)
    s = codec.encode_stream(n) if enc else codec.decode_stream(n)
    slots = [pool.open() for _ in range(capacity)][:: capacity // n][:n]     # n of the 64 open slots, spread over the state
    frames = old_frames + warmup + pushes
    if enc:
        data = torch.from_numpy((prng.normal(13, "sessions_latency", (n, frames * hop)) * 0.1).astype(np.float32)).cuda()
        piece = lambda a, m: data[:, a * hop:(a + m) * hop]      # noqa: E731
    else:
        data = torch.from_numpy(prng.randint(13, "sessions_latency", (n, frames, K), cfg.codebook_size)).to(torch.int64).cuda()
        piece = lambda a, m: data[:, a:a + m]                    # noqa: E731
    for a0 in range(0, old_frames, 26):       # every listed slot past a full window before anything is timed
        m = min(26, old_frames - a0)
        pool.push(slots, piece(a0, m))
        s.push(piece(a0, m))
    assert all(pool.frames(q) == old_frames for q in slots) and cfg.resample_stride * old_frames > cfg.sliding_window
    torch.cuda.synchronize()
    lat = {"pool": [], "stream": []}
    for i in range(warmup + pushes):
        x = piece(old_frames + i, 1)
        for who, fn in (("pool", lambda: pool.push(slots, x)), ("stream", lambda: s.push(x))):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                lat[who].append((time.perf_counter() - t0) * 1e3)
    # the mixed tick: slots[0] is a session opened just now, at position 0 beside the others' wrapped rings (one group, one native call)
    mixed = []
    for i in range(warmup + pushes):
        pool.close(slots[0])
        assert pool.open() == slots[0]
        x = piece(old_frames + i, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pool.push(slots, x)
        torch.cuda.synchronize()
        if i >= warmup:
            mixed.append((time.perf_counter() - t0) * 1e3)
    assert all(r.shape[0] == (1 if enc else hop) for r in out) and pool.frames(slots[0]) == 1
    stats = codec.profile_kernels(lambda: pool.push(slots, piece(old_frames, 1)))
    q = lambda v: (round(float(np.median(v)), 3), round(float(np.percentile(v, 99)), 3))      # noqa: E731
    (pm, pp), (sm, sp), (mm, mp) = q(lat["pool"]), q(lat["stream"]), q(mixed)
    return {"direction": direction, "capacity": capacity, "listed": n, "frames_per_push": 1, "pushes": pushes, "warmup": warmup,
            "pool_median_ms": pm, "pool_p99_ms": pp, "stream_median_ms": sm, "stream_p99_ms": sp, "pool_minus_stream_median_ms": round(pm - sm, 3),
            "mixed_tick_median_ms": mm, "mixed_tick_p99_ms": mp,
            "launches_one_pool_push": int(sum(k for _, k, _, _, _ in stats)), "kernel_ms_one_pool_push": round(sum(ms for _, _, ms, _, _ in stats), 4)}


def sessions(a):
    cfg = MIMI_24KHZ
    codec = Mimi(24000, state_dict=checkpoint.synthetic_mimi_state_dict(cfg, seed=0), config=cfg, precision=a.precision).eval()
    rows = []
    for d in ("encode", "decode"):
        for n in (1, 8, 64):
            rows.append(measure_sessions(codec, d, n, a.pushes, a.warmup))
            rows[-1]["precision"] = a.precision or "default"
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="frames (1920 samples) per push")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default=None, choices=[None, "fp32", "fp32_exact"])
    ap.add_argument("--direction", default="encode", choices=["encode", "decode"])
    ap.add_argument("--linear-route", default="auto", choices=["auto", "tap", "skinny", "ab"], help="decode only")
    ap.add_argument("--sessions", action="store_true", help="session pools of capacity 64, n = 1 / 8 / 64 listed slots, against the lockstep stream of batch n")
    ap.add_argument("--out", default=None, help="with --sessions: also write the result lines to this file as one JSON list")
    a = ap.parse_args()
    if a.sessions:
        return sessions(a)
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
