#!/usr/bin/env python3
"""Generate tests/golden/llama_score_ref.npz from the reference's own ``LlamaDecoder``.  CPU only.

    python tools/make_llama_score_golden.py --reference DIR

The fixture pins tests/llama_score_ref.py (the project's statement of teacher-forced scoring) to the reference's code: the module
DIR/downstream/models/llama3.py is imported AT GENERATION TIME, its ``LlamaDecoder`` is built for each of llama_score_ref's four
configurations -- `TINY_IN` with ``input_dim``, i.e. with the ``input`` Linear behind the embedding table --, loaded with the synthetic
weights and run in fp32 as the recipes' validation does (downstream/train_slm.py:59-92): one forward over ``embed(toks, prompt)``,
``log_softmax``, the targets' log-probabilities and the arg-max.  None of its text is stored, and no logits: the file holds the inputs
(tokens, targets, prompt), the log-probability of every target (0 at an ignored one) and the arg-max of every token row.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import llama_score_ref as SR  # noqa: E402
from make_llama_golden import reference_decoder  # noqa: E402


def build(LlamaDecoder, cfg):
    extra = {} if cfg.input_dim is None else {"input_dim": cfg.input_dim}
    m = LlamaDecoder(vocab_size=cfg.vocab_size, n_layers=cfg.n_layers, dim=cfg.dim, ffn_dim=cfg.ffn_dim, n_heads=cfg.n_heads, n_kv_heads=cfg.n_kv_heads,
                     norm_eps=cfg.norm_eps, rope_theta=cfg.rope_theta, max_seq_len=cfg.max_seq_len, prompt_dim=cfg.prompt_dim, num_codebooks=cfg.num_codebooks, **extra)
    m.load_state_dict(SR.weights(cfg), strict=True)
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    LlamaDecoder = reference_decoder(a.reference)
    B, P, T = SR.GOLDEN_SHAPE
    out, meta = {}, {"source": "downstream/models/llama3.py: LlamaDecoder (fp32, CPU)", "torch": torch.__version__, "B": B, "T": T, "cases": {}}
    with torch.no_grad():
        for name, cfg in SR.CONFIGS.items():
            m = build(LlamaDecoder, cfg)
            p = P if cfg.prompt_dim else 0
            toks, prompt, targets = SR.inputs(cfg, B, p, T)
            logits, _ = m(m.embed(toks, prompt))
            logits = logits[:, p:]
            keep = (targets >= 0) & (targets < cfg.vocab_size)
            lp = logits.log_softmax(dim=-1).gather(-1, targets.clamp(0, cfg.vocab_size - 1)[..., None])[..., 0]
            out[f"{name}_toks"], out[f"{name}_targets"] = toks.numpy().astype(np.int16), targets.numpy().astype(np.int16)
            out[f"{name}_logp"] = torch.where(keep, lp, torch.zeros_like(lp)).numpy()
            out[f"{name}_pred"] = logits.argmax(dim=-1).numpy().astype(np.int16)
            if prompt is not None:
                out[f"{name}_prompt"] = prompt.numpy()
            meta["cases"][name] = {"P": p, "scored": int(keep.sum())}
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "llama_score_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
