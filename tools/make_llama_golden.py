#!/usr/bin/env python3
"""Generate tests/golden/llama_ref.npz from the reference's own ``LlamaDecoder``.  CPU only.

    python tools/make_llama_golden.py --reference DIR

The fixture pins tests/llama_ref.py (the project's statement of the decoder) to the reference's code: the module
DIR/downstream/models/llama3.py is imported AT GENERATION TIME, its ``LlamaDecoder`` is built for each of llama_ref's three configurations,
loaded with llama_ref's synthetic weights and run in fp32.  None of its text is stored: the file holds inputs and outputs only --

    full     the logits of ``forward(embed(toks, prompt))`` over the whole sequence [B, P + T, C];
    cached   a prefill over the first P + T - STEPS rows followed by STEPS single rows through the KV cache: the logits of those
             single rows [B, STEPS, C];
    greedy   ``generate(bos, eos_id, prompt, max_gen_toks, top_p=0.0)`` with an ``eos_id`` that occurs: the rows and their lengths.

fp32 only: run in ``.double()`` the reference needs an explicit fp64 causal mask (its own fp32 mask gives logits off by 0.5), and its
RMSNorm and RoPE cast to fp32 regardless.
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import llama_ref as R  # noqa: E402

B, P, T, STEPS, GEN = 3, 6, 21, 5, 48


def reference_decoder(ref_dir):
    models = os.path.join(ref_dir, "downstream", "models")
    sys.path.insert(0, models)       # (llama3.py imports its sibling `multihead`)
    spec = importlib.util.spec_from_file_location("reference_llama3", os.path.join(models, "llama3.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.LlamaDecoder


def build(LlamaDecoder, cfg):
    m = LlamaDecoder(vocab_size=cfg.vocab_size, n_layers=cfg.n_layers, dim=cfg.dim, ffn_dim=cfg.ffn_dim, n_heads=cfg.n_heads, n_kv_heads=cfg.n_kv_heads,
                     norm_eps=cfg.norm_eps, rope_theta=cfg.rope_theta, max_seq_len=cfg.max_seq_len, prompt_dim=cfg.prompt_dim, num_codebooks=cfg.num_codebooks)
    m.load_state_dict(R.weights(cfg), strict=True)
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    LlamaDecoder = reference_decoder(a.reference)
    out, meta = {}, {"source": "downstream/models/llama3.py: LlamaDecoder (fp32, CPU)", "torch": torch.__version__, "B": B, "P": P, "T": T, "steps": STEPS, "gen": GEN, "cases": {}}
    with torch.no_grad():
        for name, cfg in R.CONFIGS.items():
            m = build(LlamaDecoder, cfg)
            p = P if cfg.prompt_dim else 0
            toks, prompt = R.inputs(cfg, B, p, T)
            embs = m.embed(toks, prompt)
            full, _ = m(embs)
            n0 = p + T - STEPS
            logits, state = m(embs[:, :n0])
            cached = []
            for i in range(n0, p + T):
                logits, state = m(embs[:, i:i + 1], state=state)
                cached.append(logits)
            bos = toks[:, :1]
            free = m.generate(bos, -1, prompt, max_gen_toks=GEN, top_p=0.0)
            eos_id = int(free[0][GEN // 3])          # occurs in row 0 at the latest there
            hyp = m.generate(bos, eos_id, prompt, max_gen_toks=GEN, top_p=0.0)
            lens = [len(h) for h in hyp]
            assert min(lens) < GEN, "the EOS id has to occur"
            rows = np.full((B, GEN), -1, dtype=np.int64)
            for i, h in enumerate(hyp):
                rows[i, :len(h)] = h.numpy()
            out[f"{name}_toks"], out[f"{name}_full"], out[f"{name}_cached"] = toks.numpy().astype(np.int16), full.numpy(), torch.cat(cached, dim=1).numpy()
            if prompt is not None:
                out[f"{name}_prompt"] = prompt.numpy()
            out[f"{name}_hyp"], out[f"{name}_free"] = rows.astype(np.int16), torch.stack(free).numpy().astype(np.int16)
            meta["cases"][name] = {"eos_id": eos_id, "lens": lens, "P": p}
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "llama_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
