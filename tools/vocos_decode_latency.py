#!/usr/bin/env python3
"""Call latency of EnCodec's `toks_to_sig` through the SEANet decoder against the Vocos decoder (`Encodec(use_vocos=True)`), eager
and with `graph=True`, on one GPU: full configurations, seeded synthetic weights, random tokens, 8 codebooks.

    python tools/vocos_decode_latency.py [--calls 200 --warmup 10] [--out profiles/vocos_decode_latency.jsonl]

One process; per shape (batch, seconds) in (1, 1), (1, 10), (64, 10) the three decoders run on the SAME tokens on alternating calls
(same clocks, same cache state).  Every call is timed on the host from the call to a stream synchronisation.  One JSON line per
shape: median / p99 (ms) of each decoder, the shader clock under the Vocos decode's tap-GEMMs, and at (64, 10) the Vocos decode's
per-kernel breakdown (`profile_kernels`).  The timed calls per decoder are `--calls` or as many as keep the fastest decoder busy for
`--window` seconds, whichever is more: no window is a fraction of a second.  Reported, not gated: there is no threshold."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiocodecs_amd import Encodec, checkpoint, prng  # noqa: E402
from audiocodecs_amd.config import ENCODEC_24KHZ, VOCOS_ENCODEC_24KHZ  # noqa: E402

SHAPES = ((1, 1), (1, 10), (64, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="least number of timed calls per decoder and shape")
    ap.add_argument("--window", type=float, default=2.0, help="least timed seconds of the fastest decoder per shape")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    cfg, vcfg = ENCODEC_24KHZ, VOCOS_ENCODEC_24KHZ
    sd = checkpoint.synthetic_state_dict(cfg, seed=0)
    vsd = checkpoint.synthetic_vocos_state_dict(vcfg, seed=0)
    kw = dict(mode="decode", num_codebooks=8, state_dict=sd, config=cfg)
    decoders = {
        "seanet": Encodec(24000, **kw).eval(),
        "vocos": Encodec(24000, use_vocos=True, vocos_state_dict=vsd, vocos_config=vcfg, **kw).eval(),
        "vocos_graph": Encodec(24000, use_vocos=True, vocos_state_dict=vsd, vocos_config=vcfg, graph=True, **kw).eval(),
    }
    lines = []
    for B, seconds in SHAPES:
        N = seconds * cfg.frame_rate
        calls = a.calls
        toks = torch.from_numpy(prng.randint(17, f"vocos_latency_{B}_{seconds}", (B, N, 8), cfg.codebook_size)).to(torch.int64).cuda()
        lat = {k: [] for k in decoders}
        i, warm = 0, []
        while i < a.warmup + calls:
            for name, codec in decoders.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sig = codec.toks_to_sig(toks)
                torch.cuda.synchronize()
                (lat[name] if i >= a.warmup else warm).append((time.perf_counter() - t0) * 1e3)
            assert sig.shape == (B, N * cfg.hop_length)
            i += 1
            if i == a.warmup:     # size the timed window from the fastest warm call
                calls = max(a.calls, int(a.window * 1e3 / min(warm)) + 1)
        row = {"batch": B, "seconds": seconds, "frames": N, "calls": calls, "warmup": a.warmup}
        for name, v in lat.items():
            row[f"{name}_median_ms"] = round(float(np.median(v)), 3)
            row[f"{name}_p99_ms"] = round(float(np.percentile(v, 99)), 3)
        voc = decoders["vocos"]
        nat = next(iter(voc._vocos_natives.values()))
        mhz = C.c_double(0.0)
        nat.lib.ac_debug_clock(nat.h, 1, C.byref(mhz))
        voc.toks_to_sig(toks)
        torch.cuda.synchronize()
        nat.lib.ac_debug_clock(nat.h, 0, C.byref(mhz))
        row["vocos_shader_mhz"] = round(mhz.value, 0)
        if (B, seconds) == SHAPES[-1]:
            stats = voc.profile_kernels(lambda: voc.toks_to_sig(toks))
            row["vocos_kernels"] = [{"name": n, "launches": k, "ms": round(ms, 4), "tflops": round(fl / ms / 1e9, 1) if ms > 0 else None}
                                    for n, k, ms, fl, _ in sorted(stats, key=lambda r: -r[2])]
        print(json.dumps(row), flush=True)
        lines.append(json.dumps(row))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
