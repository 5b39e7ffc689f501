#!/usr/bin/env python3
"""Generate tests/golden/token_probe_ref.npz from the reference's own embedding and pooling modules.  CPU only.

    python tools/make_token_probe_golden.py --reference DIR

The fixture pins the front of tests/token_probe_ref.py (the project's statement of the TokenProbe) to the reference's code: the modules
DIR/downstream/models/multihead.py and pooling.py are imported AT GENERATION TIME; ``MultiHeadEmbedding`` (without and with
``padding_idx``), ``LinearPooling`` and ``AttentionalPooling`` are built for token_probe_ref's tiny configurations, loaded with the
synthetic weights and run in fp32.  None of their text is stored: the file holds the token ids and the pooled rows.
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

import token_probe_ref as PR  # noqa: E402

GOLDEN_CASES = {"linear": "TINY", "attentional_padded": "TINY_ATT"}      # fixture key -> token_probe_ref configuration
GOLDEN_SHAPE = (3, 37)


def load(reference, name):
    path = os.path.join(reference, "downstream", "models", name + ".py")
    spec = importlib.util.spec_from_file_location("reference_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    mh, pl = load(a.reference, "multihead"), load(a.reference, "pooling")
    B, N = GOLDEN_SHAPE
    out, meta = {}, {"source": "downstream/models/multihead.py: MultiHeadEmbedding; pooling.py: LinearPooling, AttentionalPooling (fp32, CPU)",
                     "torch": torch.__version__, "cases": {}}
    with torch.no_grad():
        for key, cname in GOLDEN_CASES.items():
            cfg = PR.CONFIGS[cname]
            sd = PR.weights(cfg)
            emb = mh.MultiHeadEmbedding(cfg.vocab_size, cfg.embedding_dim, cfg.num_codebooks, padding_idx=cfg.padding_idx)
            emb.weight.copy_(sd["embedding.weight"])
            if cfg.pooling == "linear":
                pool = pl.LinearPooling(cfg.num_codebooks)
                pool.mlp.weight.copy_(sd["pooling.mlp.weight"])
            else:
                pool = pl.AttentionalPooling(cfg.embedding_dim)
                pool.load_state_dict({k[len("pooling."):]: v for k, v in sd.items() if k.startswith("pooling.")}, strict=True)
            toks = PR.inputs(cfg, B, N)
            pooled = pool(emb(toks.clone()))
            out[f"{key}_toks"], out[f"{key}_pooled"] = toks.numpy().astype(np.int16), pooled.numpy().astype(np.float32)
            meta["cases"][key] = {"config": cname, "padded_ids": int((toks == cfg.vocab_size).sum())}
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "token_probe_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
