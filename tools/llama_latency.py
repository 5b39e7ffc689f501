#!/usr/bin/env python3
"""Time per generated token of `LlamaDecoder.generate` against the torch statement of the same decoder with its KV cache, on one GPU.

    python tools/llama_latency.py [--batches 1 8 32 --prompt 64 --steps 1500 --calls 3 --warmup 1] [--out profiles/llama_latency.jsonl]

`LLAMA_TTS` (12 layers, dim 512, 4 query heads over 1 key/value head of 128, ffn 2048, vocabulary 1026, 2 codebooks) with seeded random
weights, a prompt of 64 rows, 1500 generated tokens, top_p = 0.9, eos_id = -1 (every row runs all steps).  One process, one JSON line per
batch size; the two forms run on alternating calls (latency_common):
    fused   `LlamaDecoder.generate`: prefill, then replays of the captured graph of steps;
    torch   tests/llama_ref.py's `Statement` in fp32 on the GPU, the cache allocated once, and the reference's per-token chain
            (llama3.py:947-977): log_softmax, sort, cumsum, mask, multinomial, gather, and `alive.any()` on the host.
Each line carries ms per generated token of both forms (the host clock around a whole call up to a synchronise, over the steps), the
library's launches per step and the share of one weight pass: the bytes of every weight a step reads, over the step time, over the
4.7 TB/s this project measured as its memory skeleton.  Reported, not gated: there is no threshold."""
import argparse
import dataclasses
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import llama_ref as R  # noqa: E402
from audiocodecs_amd import LLAMA_TTS, LlamaDecoder  # noqa: E402
from audiocodecs_amd.llama import weight_names  # noqa: E402
from latency_common import alternate, emit, median_p99  # noqa: E402

TOP_P, TEMP, SKELETON = 0.9, 1.0, 4.7e12


def random_weights(cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name in weight_names(cfg):
        shape = R._shape(cfg, name)
        x = torch.randn(shape, generator=g)
        sd[name] = 1.0 + 0.1 * x if len(shape) == 1 else x if name == "tok_embeddings.weight" else x * (R.W_SCALE / (3.0 * shape[1]) ** 0.5)
    return sd


def step_weight_bytes(cfg):
    """What one generated token reads of the weights: every layer matrix, one output head, one embedding row per batch entry aside."""
    hd = cfg.head_dim
    layer = (cfg.n_heads + 2 * cfg.n_kv_heads) * hd * cfg.dim + cfg.dim * cfg.n_heads * hd + 3 * cfg.ffn * cfg.dim + 2 * cfg.dim
    return 4 * (cfg.n_layers * layer + cfg.vocab_size * cfg.dim + cfg.dim)


def launches_per_step(cfg):
    return 2 + 6 * cfg.n_layers + 1      # sampler, bookkeeping; per layer qkv, attention, combine, wo, w1|w3, w2; head


def torch_generate(stmt, bos, prompt, steps):
    """The reference's loop on the statement: top-p by its chain of torch operations, `alive.any()` read on the host every token."""
    stmt.reset()
    B = bos.shape[0]
    embs = stmt.embed(bos, prompt)
    hyp = torch.full((B, steps), -1, device=bos.device)
    alive = torch.ones(B, dtype=torch.bool, device=bos.device)
    lens = torch.zeros(B, device=bos.device)
    n = 0
    while n < steps:
        logits = stmt.forward(embs)[:, -1]
        probs = (logits / TEMP).log_softmax(dim=-1).exp()
        probs, idx = probs.sort(dim=-1, descending=True)
        probs[probs.cumsum(dim=-1) - probs > TOP_P] = 0.0
        probs = probs / probs.sum(dim=-1, keepdim=True)
        tok = idx.gather(-1, torch.multinomial(probs, num_samples=1))[:, 0]
        hyp[:, n] = tok
        alive = alive & (tok != -1)
        lens[alive] += 1
        n += 1
        if not alive.any():
            break
        embs = stmt.embed(tok[:, None], curr_pos=n)
    return hyp


def measure(B, a, cfg, sd, dec):
    g = torch.Generator().manual_seed(B)
    bos = torch.randint(0, cfg.vocab_size, (B, 1), generator=g).cuda()
    prompt = torch.randn(B, a.prompt, cfg.prompt_dim, generator=g).cuda()
    stmt = R.Statement(cfg, sd, torch.float32, device="cuda", capacity=a.prompt + 1 + a.steps)
    seed = [0]

    def fused():
        seed[0] += 1
        return dec.generate(bos, -1, prompt, max_gen_toks=a.steps, top_p=TOP_P, temp=TEMP, seed=seed[0])

    forms = {"fused": fused, "torch": lambda: torch_generate(stmt, bos, prompt, a.steps)}
    with torch.no_grad():
        alternate(forms, dict.fromkeys(forms, a.warmup))
        lat, last = alternate(forms, dict.fromkeys(forms, a.calls))
    per = {k: [ms / a.steps for ms in v] for k, v in lat.items()}
    fused_s = float(sorted(per["fused"])[len(per["fused"]) // 2]) * 1e-3
    ok = all(len(r) == a.steps for r in last["fused"]) and bool(((torch.stack(last["fused"]) >= 0) & (torch.stack(last["fused"]) < cfg.vocab_size)).all())
    return {"what": "llama_generate", "model": "LLAMA_TTS", "B": B, "prompt": a.prompt, "steps": a.steps, "top_p": TOP_P, "calls": a.calls,
            **median_p99(per["fused"], 4, "fused_token_"), **median_p99(per["torch"], 4, "torch_token_"),
            "launches_per_step": launches_per_step(cfg), "weight_bytes_per_step": step_weight_bytes(cfg),
            "share_of_weight_pass": round(step_weight_bytes(cfg) / SKELETON / fused_s, 4), "tokens_in_range": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--prompt", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--calls", type=int, default=3, help="timed calls per form and batch size")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("llama_latency: no GPU: a timing needs one")
    cfg = dataclasses.replace(LLAMA_TTS, prompt_dim=512)
    sd = random_weights(cfg)
    dec = LlamaDecoder(state_dict=sd, config=cfg)
    for B in a.batches:
        emit(measure(B, a, cfg, sd, dec), a.out)


if __name__ == "__main__":
    main()
