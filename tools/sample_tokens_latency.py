#!/usr/bin/env python3
"""Time of the fused `sample_tokens` against the reference's sampling chain as torch ops, and of the fused `Codec.resample(seed=0)` against the
torch `Codec.resample`, on one GPU.

    python tools/sample_tokens_latency.py [--calls 200 --window 0.5 --max-calls 2000 --warmup 5 --resample-calls 10] [--out profiles/sample_tokens_latency.jsonl]

One process, one JSON line per measurement.  The forms of a measurement run on the SAME data on alternating calls (latency_common):
    sample    [B, C] in {1, 8, 64} x {1025, 4097} logits, top_p = 0.9, temp = 1:
              fused   `sample_tokens(logits, top_p=0.9, seed=0, offset=i)`: one launch;
              torch   downstream/models/llama3.py:952-996 per generated token: log_softmax, exp, sort, cumsum, mask, renormalise,
                      multinomial, gather.
    resample  [64, 750, 8] tokens on the full-size EnCodec with seeded random weights (C = 1024), p = 0.2:
              fused   `codec.resample(toks, seed=0)`;
              torch   `codec.resample(toks)`: a [384 000, 1024] gather, softmax and multinomial.
Each line carries the median and the p99 of both forms on the host clock up to a synchronise, and the shader clock sampled while calls
are queued.  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiocodecs_amd import sample_tokens  # noqa: E402
from latency_common import alternate, alternate_for, emit, median_p99, shader_mhz  # noqa: E402

SHAPES = [(B, C) for C in (1025, 4097) for B in (1, 8, 64)]
TOP_P = 0.9


def torch_chain(logits, temp, p):
    """What the reference's generator does with the last position's logits for one token (llama3.py:952, 961-962, 986-996)."""
    probs = (logits / temp).log_softmax(dim=-1).exp()
    probs, idx = probs.sort(dim=-1, descending=True)
    probs_sum = probs.cumsum(dim=-1)
    probs[probs_sum - probs > p] = 0.0
    probs = probs / probs.sum(dim=-1, keepdim=True)
    return idx.gather(-1, torch.multinomial(probs, num_samples=1))[:, 0]


def queued_clock(fn, n=20):
    for _ in range(n):
        fn()
    mhz = shader_mhz()
    torch.cuda.synchronize()
    return mhz


def measure_sample(B, C, a):
    logits = (3.0 * torch.randn(B, C, generator=torch.Generator().manual_seed(B * C))).cuda()
    step = [0]

    def fused():
        step[0] += B
        return sample_tokens(logits, top_p=TOP_P, seed=0, offset=step[0])

    forms = {"fused": fused, "torch": lambda: torch_chain(logits, 1.0, TOP_P)}
    lat, last, calls = alternate_for(forms, a.calls, a.window, a.max_calls, a.warmup)
    in_range = bool(((last["fused"] >= 0) & (last["fused"] < C)).all())
    return {"what": "sample", "B": B, "C": C, "top_p": TOP_P, "calls": calls, **median_p99(lat["fused"], 4, "fused_"), **median_p99(lat["torch"], 4, "torch_"),
            "shader_mhz": queued_clock(fused), "tokens_in_range": in_range}


def measure_resample(a):
    from audiocodecs_amd import Encodec, checkpoint
    from audiocodecs_amd.config import ENCODEC_24KHZ as cfg

    codec = Encodec(24000, num_codebooks=8, state_dict=checkpoint.synthetic_state_dict(cfg, seed=0)).eval()
    B, N, K = 64, 750, 8
    toks = torch.randint(0, cfg.codebook_size, (B, N, K), generator=torch.Generator().manual_seed(1)).cuda()
    codec.logits()      # (the cached table: built once, outside the timing)
    forms = {"fused": lambda: codec.resample(toks, seed=0), "torch": lambda: codec.resample(toks)}
    alternate(forms, dict.fromkeys(forms, max(1, a.warmup // 2)))
    lat, last = alternate(forms, dict.fromkeys(forms, a.resample_calls))
    changed = {name: round(float((out != toks).float().mean()), 4) for name, out in last.items()}
    return {"what": "resample", "codec": "encodec_24khz", "B": B, "N": N, "K": K, "C": cfg.codebook_size, "p": 0.2, "calls": a.resample_calls,
            **median_p99(lat["fused"], 4, "fused_"), **median_p99(lat["torch"], 4, "torch_"), "shader_mhz": queued_clock(forms["fused"], 5),
            "share_changed": changed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200, help="least calls per form of a sample shape")
    ap.add_argument("--window", type=float, default=0.5, help="seconds the faster form is kept busy")
    ap.add_argument("--max-calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--resample-calls", type=int, default=10)
    ap.add_argument("--no-resample", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    for B, C in SHAPES:
        emit(measure_sample(B, C, a), a.out)
    if not a.no_resample:
        emit(measure_resample(a), a.out)


if __name__ == "__main__":
    main()
