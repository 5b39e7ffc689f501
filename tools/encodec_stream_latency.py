#!/usr/bin/env python3
"""Push latency of streaming EnCodec encode (Encodec.encode_stream) or decode (Encodec.decode_stream) on one GPU: EnCodec 24 kHz,
seeded synthetic weights, noise input / random tokens.

    python tools/encodec_stream_latency.py --batch 1 --frames 1 [--pushes 200 --warmup 20] [--direction decode]
    python tools/encodec_stream_latency.py --sweep [--out profiles/encodec_stream_latency.json]
    python tools/encodec_stream_latency.py --sweep --sample-rate 16000 --out profiles/encodec_stream_latency_16k.json
    python tools/encodec_stream_latency.py --sessions --out profiles/encodec_sessions_latency.json
    python tools/encodec_stream_latency.py --sessions --sample-rate 16000 --out profiles/encodec_sessions_latency_16k.json

Same method as tools/mimi_stream_latency.py: after the stream's own start-up hold (one push of WARMUP_FRAMES frames, not timed) and
`--warmup` untimed pushes, every push is timed on the host from `push` to a stream synchronisation (what a caller waiting for its
tokens sees).  Prints one JSON line per configuration: median / p99 push latency (ms), the real-time factor (audio seconds per
compute second, per stream and batch-wide), the per-kernel split of ONE further push (Encodec.profile_kernels: HIP-event time per
kernel name, launches) and, for scale, the one-shot time of a 10 s clip at the same batch size (`sig_to_toks` / `toks_to_sig`, median
of 5): what a caller without streaming pays for every new frame.  `--sweep` runs B = 1 / 8 / 64 with one-frame and 25-frame pushes
in both directions; `--out` also writes the lines as one JSON list.

`--sample-rate R` (R != 24000) measures the caller at another rate: every configuration runs twice in the same process, as the plain
24 kHz stream ("resample": false) and as `encode_stream / decode_stream(B, resample=True)` of a codec built for rate R ("resample":
true), whose pushes carry the same audio time (F frames; at 16 kHz an encode push is 213 or 214 samples per frame) and pass the
stateful resampler (ResampleStream: two launches per push, not on a handle, so not in the per-kernel split).  The difference of the
two medians is the resampler's cost per push.

`--sessions` measures session pools (Encodec.encode_sessions / decode_sessions): a pool of capacity 64 with
n = 1 / 8 / 64 listed slots against the lockstep stream of batch n, one-frame pushes in both directions.  The two run in one process
on ALTERNATING pushes (pool, stream, pool, ...), so that clock and cache state are shared; after each one's start-up release and
`--warmup` untimed pushes, `--pushes` pushes of each are timed as above.  "mixed tick" is the pool's push in which one listed slot
releases its 7 held frames beside n - 1 steady slots (two native calls; the slot is closed, reopened and fed 6 frames, untimed, before
every timed push).  Nothing is gated on these numbers: the lockstep stream at the same n is the baseline of a subset push.

`--sessions --sample-rate R` (R != 24000) also times the resampling pool (`encode_sessions / decode_sessions(64, resample=True)` of a
codec built for rate R) against the plain 24 kHz pool at the same n, again on alternating pushes in one process.
The pushes cover the same audio time, one frame: at 16 kHz an encode push is 213 or 214 samples, of which the resampler completes 318
to 321, so a push of the resampling pool runs one frame most of the time and none or two now and then, as a caller's would.  The
difference of the two medians is what the per-slot resampler costs per push (one host-to-device copy and two launches)."""
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


def measure(codec, direction, B, F, pushes, warmup, resample=False):
    cfg = codec.config
    hop, K = cfg.hop_length, codec.num_codebooks
    s = codec.encode_stream(B, resample=resample) if direction == "encode" else codec.decode_stream(B, resample=resample)
    rate = int(codec.sample_rate)                    # the caller's rate: the codec's own unless resampling
    W = s.WARMUP_FRAMES + (1 if resample else 0)     # (resampling: one frame more, the resampler holds the last 0.5 ms back)
    total = warmup + pushes + 1                      # + 1: the profiled push
    frames = W + total * F
    if direction == "encode":
        at = lambda a: (a * hop * rate + cfg.sampling_rate // 2) // cfg.sampling_rate       # noqa: E731  (frame a's first sample at `rate`)
        data = torch.from_numpy((prng.normal(11, "stream_latency", (B, at(frames))) * 0.1).astype(np.float32)).cuda()
        piece = lambda a, n: data[:, at(a):at(a + n)]            # noqa: E731
    else:
        data = torch.from_numpy(prng.randint(11, "stream_latency", (B, frames, K), cfg.codebook_size)).to(torch.int64).cuda()
        piece = lambda a, n: data[:, a:a + n]                    # noqa: E731
    first = s.push(piece(0, W))                      # the start-up hold, released as one push
    assert resample or first.shape[1] == (W if direction == "encode" else W * hop)
    assert first.shape[1] > 0
    torch.cuda.synchronize()
    lat = []
    for i in range(warmup + pushes):
        t0 = time.perf_counter()
        out = s.push(piece(W + i * F, F))
        torch.cuda.synchronize()
        if i >= warmup:
            lat.append(time.perf_counter() - t0)
    assert resample or out.shape[1] == (F if direction == "encode" else F * hop)
    stats = codec.profile_kernels(lambda: s.push(piece(W + (warmup + pushes) * F, F)))
    lat = np.array(lat) * 1e3
    med = float(np.median(lat))
    audio_ms = F * hop / cfg.sampling_rate * 1e3
    # the one-shot path on a 10 s clip at the same batch size
    n10 = 10 * cfg.sampling_rate // hop
    if direction == "encode":
        clip = torch.from_numpy((prng.normal(12, "stream_latency", (B, n10 * hop * rate // cfg.sampling_rate)) * 0.1).astype(np.float32)).cuda()
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


def measure_sessions(codec, direction, n, pushes, warmup, capacity=64):
    cfg = codec.config
    hop, K = cfg.hop_length, codec.num_codebooks
    enc = direction == "encode"
    pool = codec.encode_sessions(capacity) if enc else codec.decode_sessions(capacity)
    s = codec.encode_stream(n) if enc else codec.decode_stream(n)
    W = pool.WARMUP_FRAMES
    slots = [pool.open() for _ in range(capacity)][:: capacity // n][:n]     # n of the 64 open slots, spread over the state
    frames = W + warmup + pushes
    if enc:
        data = torch.from_numpy((prng.normal(13, "sessions_latency", (n, frames * hop)) * 0.1).astype(np.float32)).cuda()
        piece = lambda a, m: data[:, a * hop:(a + m) * hop]      # noqa: E731
    else:
        data = torch.from_numpy(prng.randint(13, "sessions_latency", (n, frames, K), cfg.codebook_size)).to(torch.int64).cuda()
        piece = lambda a, m: data[:, a:a + m]                    # noqa: E731
    unit = hop if enc else 1
    first = pool.push(slots, piece(0, W))
    assert all(r.shape[0] == (W if enc else W * hop) for r in first) and s.push(piece(0, W)).shape[1] == first[0].shape[0]
    torch.cuda.synchronize()
    lat = {"pool": [], "stream": []}
    for i in range(warmup + pushes):
        x = piece(W + i, 1)
        for who, fn in (("pool", lambda: pool.push(slots, x)), ("stream", lambda: s.push(x))):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                lat[who].append((time.perf_counter() - t0) * 1e3)
    # the mixed tick: slots[0] is a new session that releases its hold beside the others' one frame
    mixed = []
    for i in range(warmup + pushes):
        pool.close(slots[0])
        assert pool.open() == slots[0]
        held = pool.push(slots[:1], piece(0, W - 1)[:1])
        assert held[0].shape[0] == 0 and pool.pending(slots[0]) == (W - 1) * unit
        x = piece(W + i, 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = pool.push(slots, x)
        torch.cuda.synchronize()
        if i >= warmup:
            mixed.append((time.perf_counter() - t0) * 1e3)
    assert out[0].shape[0] == (W if enc else W * hop) and all(r.shape[0] == (1 if enc else hop) for r in out[1:])
    stats = codec.profile_kernels(lambda: pool.push(slots, piece(W, 1)))
    q = lambda v: (round(float(np.median(v)), 3), round(float(np.percentile(v, 99)), 3))      # noqa: E731
    (pm, pp), (sm, sp), (mm, mp) = q(lat["pool"]), q(lat["stream"]), q(mixed)
    return {"direction": direction, "capacity": capacity, "listed": n, "frames_per_push": 1, "pushes": pushes, "warmup": warmup,
            "pool_median_ms": pm, "pool_p99_ms": pp, "stream_median_ms": sm, "stream_p99_ms": sp, "pool_minus_stream_median_ms": round(pm - sm, 3),
            "mixed_tick_median_ms": mm, "mixed_tick_p99_ms": mp,
            "launches_one_pool_push": int(sum(k for _, k, _, _, _ in stats)), "kernel_ms_one_pool_push": round(sum(ms for _, _, ms, _, _ in stats), 4)}


def measure_sessions_resampled(codec, codec_r, direction, n, pushes, warmup, capacity=64):
    """The resampling pool of `codec_r` (the caller's rate) against the plain pool of `codec` at the same n, alternating."""
    cfg = codec.config
    hop, K, rate = cfg.hop_length, codec.num_codebooks, int(codec_r.sample_rate)
    enc = direction == "encode"
    pools = {"plain": codec.encode_sessions(capacity) if enc else codec.decode_sessions(capacity),
             "resampling": codec_r.encode_sessions(capacity, resample=True) if enc else codec_r.decode_sessions(capacity, resample=True)}
    W = pools["plain"].WARMUP_FRAMES + 1            # (one frame more: the resampler holds the last 0.5 ms back)
    slots = {who: [p.open() for _ in range(capacity)][:: capacity // n][:n] for who, p in pools.items()}
    frames = W + warmup + pushes
    if enc:
        at = {"plain": lambda a: a * hop, "resampling": lambda a: (a * hop * rate + cfg.sampling_rate // 2) // cfg.sampling_rate}
        data = {who: torch.from_numpy((prng.normal(14, "sessions_latency", (n, at[who](frames))) * 0.1).astype(np.float32)).cuda() for who in pools}
        piece = lambda who, a, m: data[who][:, at[who](a):at[who](a + m)]      # noqa: E731
    else:
        toks = torch.from_numpy(prng.randint(14, "sessions_latency", (n, frames, K), cfg.codebook_size)).to(torch.int64).cuda()
        piece = lambda who, a, m: toks[:, a:a + m]                # noqa: E731
    for who, p in pools.items():
        assert all(r.shape[0] > 0 for r in p.push(slots[who], piece(who, 0, W)))      # the start-up hold, released as one push
    torch.cuda.synchronize()
    lat = {who: [] for who in pools}
    for i in range(warmup + pushes):
        for who, p in pools.items():
            x = piece(who, W + i, 1)
            t0 = time.perf_counter()
            p.push(slots[who], x)
            torch.cuda.synchronize()
            if i >= warmup:
                lat[who].append((time.perf_counter() - t0) * 1e3)
    q = lambda v: (round(float(np.median(v)), 3), round(float(np.percentile(v, 99)), 3))      # noqa: E731
    (pm, pp), (rm, rp) = q(lat["plain"]), q(lat["resampling"])
    return {"direction": direction, "capacity": capacity, "listed": n, "frames_per_push": 1, "pushes": pushes, "warmup": warmup, "sample_rate": rate,
            "plain_pool_median_ms": pm, "plain_pool_p99_ms": pp, "resampling_pool_median_ms": rm, "resampling_pool_p99_ms": rp,
            "resampling_minus_plain_median_ms": round(rm - pm, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--frames", type=int, default=1, help="frames (320 samples) per push")
    ap.add_argument("--pushes", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--precision", default=None, choices=[None, "fp32", "fp32_exact"])
    ap.add_argument("--direction", default="encode", choices=["encode", "decode"])
    ap.add_argument("--sweep", action="store_true", help="B = 1 / 8 / 64 x 1 / 25 frames per push x both directions")
    ap.add_argument("--sessions", action="store_true", help="session pools of capacity 64, n = 1 / 8 / 64 listed slots, against the lockstep stream of batch n")
    ap.add_argument("--out", default=None, help="also write the result lines to this file as one JSON list")
    ap.add_argument("--sample-rate", type=int, default=24000, help="the caller's rate; another one than 24000 also runs every configuration with resample=True")
    a = ap.parse_args()
    cfg = ENCODEC_24KHZ
    sd = checkpoint.synthetic_state_dict(cfg, seed=0)
    codec = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg, precision=a.precision).eval()
    runs = [(d, B, F) for d in ("encode", "decode") for B in (1, 8, 64) for F in (1, 25)] if a.sweep else [(a.direction, a.batch, a.frames)]
    variants = [(codec, False)]
    if a.sample_rate != cfg.sampling_rate:
        variants.append((Encodec(a.sample_rate, num_codebooks=8, state_dict=sd, config=cfg, precision=a.precision).eval(), True))
    rows = []
    if a.sessions:
        runs = []
        for d in ("encode", "decode"):
            for n in (1, 8, 64):
                rows.append(measure_sessions(codec, d, n, a.pushes, a.warmup))
                rows[-1]["precision"] = a.precision or "default"
                print(json.dumps(rows[-1]), flush=True)
                if len(variants) > 1:
                    rows.append(measure_sessions_resampled(codec, variants[1][0], d, n, a.pushes, a.warmup))
                    rows[-1]["precision"] = a.precision or "default"
                    print(json.dumps(rows[-1]), flush=True)
    for d, B, F in runs:
        for c, rs in variants:
            rows.append(measure(c, d, B, F, a.pushes, a.warmup, rs))
            rows[-1]["precision"] = a.precision or "default"
            if len(variants) > 1:
                rows[-1].update(sample_rate=int(c.sample_rate), resample=rs)
            print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
