#!/usr/bin/env python3
"""Time of one teacher-forced scoring pass of `LlamaDecoder.score` against what the library offered before it and against the torch
statement, on one GPU.

    python tools/llama_score_latency.py [--batches 1 4 16 --toks 6001 --calls 3 --warmup 1 --forms score forward torch] [--out FILE.jsonl]

The recipe model with seeded random weights: 12 layers, dim 512, 4 query heads over 1 key/value head of 128, ffn 2048, vocabulary 1026,
8 codebooks, max_seq_len 8192.  T = 6001 positions (a bos token and a 10 s clip of EnCodec at 8 codebooks), no prompt.  One process, one
JSON line per batch size; the forms run on alternating calls (latency_common), each timed on the host clock from an idle device to an idle
device, `--calls` timed calls behind `--warmup` untimed ones:
    score     `LlamaDecoder.score(toks, targets)`;
    forward   what the library offered before: `embed` + `forward` (the fp32 path built for prefill, its logits in memory) + torch
              `log_softmax`, `gather`, `argmax` and the sums on the same GPU;
    torch     tests/llama_ref.py's statement in fp32 on the GPU + the same torch operations.
Each line also carries the two floors of `score` computed from the shapes -- one pass over the packed weights at the 4.7 TB/s this project
measured as its memory skeleton, and the matrix products (3 fp16 products per fp32 product, the attention's lower triangle) at the chip's
2.5 PFLOP/s fp16 rate -- as shares of the measured median.  Reported, not gated: there is no threshold."""
import argparse
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import llama_ref as R  # noqa: E402
import llama_score_ref as SR  # noqa: E402
from audiocodecs_amd import LLAMA_TTS, LlamaDecoder  # noqa: E402
from latency_common import alternate, emit, median_p99  # noqa: E402
from llama_latency import random_weights  # noqa: E402

SKELETON, MFMA_PEAK = 4.7e12, 2.5e15
CFG = dataclasses.replace(LLAMA_TTS, num_codebooks=8, max_seq_len=8192)


def weight_bytes(cfg):
    """What one pass reads of the packed weights: every layer matrix as two fp16 planes (4 bytes per weight), every output head."""
    hd = cfg.head_dim
    layer = (cfg.n_heads + 2 * cfg.n_kv_heads) * hd * cfg.dim + cfg.dim * cfg.n_heads * hd + 3 * cfg.ffn * cfg.dim
    return 4 * (cfg.n_layers * layer + cfg.num_codebooks * cfg.vocab_size * cfg.dim)


def mfma_flops(cfg, B, T):
    """fp16 matrix-pipe operations of one pass: 3 products per fp32 product; the attention over the causal half."""
    hd = cfg.head_dim
    layer = 2.0 * B * T * ((cfg.n_heads + 2 * cfg.n_kv_heads) * hd * cfg.dim + cfg.dim * cfg.n_heads * hd + 3 * cfg.ffn * cfg.dim)
    attn = 2.0 * 2.0 * B * cfg.n_heads * hd * (T * (T + 1) / 2)
    return 3.0 * (cfg.n_layers * (layer + attn) + 2.0 * B * T * cfg.vocab_size * cfg.dim)


def torch_score(logits, targets):
    s = SR.score(logits, targets)
    return s["logp"], s["pred"], s["sum_logp"], s["count"], s["errors"]


def measure(B, a, dec, stmt):
    g = torch.Generator().manual_seed(B)
    toks = torch.randint(0, CFG.vocab_size, (B, a.toks), generator=g).cuda()
    targets = torch.randint(0, CFG.vocab_size, (B, a.toks), generator=g).cuda()

    def forward():
        logits, _ = dec.forward(dec.embed(toks), capacity=a.toks)
        return torch_score(logits, targets)

    def statement():
        stmt.reset()
        return torch_score(stmt.forward(stmt.embed(toks)), targets)

    def score():
        s = dec.score(toks, targets)
        return s.logp, s.pred, s.sum_logp, s.count, s.errors

    forms = {k: v for k, v in {"score": score, "forward": forward, "torch": statement}.items() if k in a.forms}
    with torch.no_grad():
        alternate(forms, dict.fromkeys(forms, a.warmup))
        lat, last = alternate(forms, dict.fromkeys(forms, a.calls))
    row = {"what": "llama_score", "B": B, "T": a.toks, "calls": a.calls, "forms": list(forms)}
    for k in forms:
        row.update(median_p99(lat[k], 2, k + "_"))
    if "score" in forms:
        sec = row["score_median_ms"] * 1e-3
        row.update({"weight_bytes": weight_bytes(CFG), "share_of_weight_pass": round(weight_bytes(CFG) / SKELETON / sec, 5), "mfma_flops": mfma_flops(CFG, B, a.toks),
                    "share_of_mfma_floor": round(mfma_flops(CFG, B, a.toks) / MFMA_PEAK / sec, 4)})
        for k in forms:
            if k != "score":            # the forms agree: the worst log-prob difference and the share of equal arg-maxes
                row[f"{k}_logp_diff"] = float((last[k][0] - last["score"][0]).abs().max())
                row[f"{k}_pred_equal"] = round(float((last[k][1] == last["score"][1]).double().mean()), 6)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--toks", type=int, default=6001)
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form and batch size")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--forms", nargs="+", default=["score", "forward", "torch"], choices=["score", "forward", "torch"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("llama_score_latency: no GPU: a timing needs one")
    sd = random_weights(CFG)
    dec = LlamaDecoder(state_dict=sd, config=CFG)
    stmt = R.Statement(CFG, sd, torch.float32, device="cuda") if "torch" in a.forms else None
    for B in a.batches:
        emit(measure(B, a, dec, stmt), a.out)


if __name__ == "__main__":
    main()
