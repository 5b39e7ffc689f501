#!/usr/bin/env python3
"""Generate tests/golden/mimi_stream_golden.npz: transformers' MimiModel streaming encode (build container only).

    python tools/make_golden_mimi_stream.py

What runs: ``transformers.MimiModel(hf_mimi_config(cfg))`` holding OUR seeded synthetic weights
(audiocodecs_amd.checkpoint.synthetic_mimi_state_dict), encoded with ``use_streaming=True`` in the whole-frame pushes of
tests/mimi_stream_cases.py, carrying its conv padding cache and transformer KV cache from push to push.  Stored per case:
  <name>_stream   HF's streamed tokens [B, N, K] (int16)
  <name>_oneshot  HF's one-shot ``encode`` of the same signal (int16)
  <name>_margin   the fp64 oracle's relative margins of the same signal (float32; near-tie audit, tests/test_oracle_golden.py)
and the push schedule of every case in the meta JSON.  Inputs are NOT stored (re-drawn by mimi_stream_cases.make_signal).
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import checkpoint  # noqa: E402
from audiocodecs_amd.config import MIMI_24KHZ, MIMI_TINY  # noqa: E402
from mimi_stream_cases import CASES, HOP, make_signal, pushes  # noqa: E402
from oracle import mimi_oracle as O  # noqa: E402
from reference_shim import hf_mimi_config  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
K = 8


def hf_model(cfg, sd):
    from transformers import MimiModel

    m = MimiModel(hf_mimi_config(cfg)).eval()
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "rotary_emb" not in k]
    if missing or unexpected:
        raise RuntimeError(f"state dict mismatch: missing {missing[:4]}, unexpected {unexpected[:4]}")
    return m


def main():
    import transformers

    torch.set_num_threads(8)
    out = {}
    meta = {"transformers": transformers.__version__, "torch": torch.__version__, "K": K, "hop": HOP, "cases": {}}
    models = {}
    for case in CASES:
        name, cfg_name, seed = case["name"], case["cfg"], case["weights_seed"]
        cfg = {"full": MIMI_24KHZ, "tiny": MIMI_TINY}[cfg_name]
        if (cfg_name, seed) not in models:
            sd = checkpoint.synthetic_mimi_state_dict(cfg, seed=seed)
            models[(cfg_name, seed)] = (hf_model(cfg, sd), O.cast_weights(sd, torch.float64))
        model, W64 = models[(cfg_name, seed)]
        sig = torch.from_numpy(make_signal(case, GOLD))
        frames = sig.shape[1] // HOP
        sched = pushes(case, frames)
        with torch.no_grad():
            pkv, pc, parts, t = None, None, [], 0
            for n in sched:
                o = model.encode(sig[:, None, t * HOP:(t + n) * HOP], num_quantizers=K, use_streaming=True,
                                 padding_cache=pc, encoder_past_key_values=pkv, return_dict=True)
                pkv, pc = o.encoder_past_key_values, o.padding_cache
                parts.append(o.audio_codes.movedim(-1, -2))
                t += n
            stream = torch.cat(parts, 1)
            oneshot = model.encode(sig[:, None], num_quantizers=K, return_dict=True).audio_codes.movedim(-1, -2)
            _, margin = O.sig_to_toks(cfg, W64, sig.double(), None, K, True)
        assert stream.shape == oneshot.shape == margin.shape == (sig.shape[0], frames, K), (stream.shape, oneshot.shape, margin.shape)
        ndiff = int((stream != oneshot).sum())
        out[f"{name}_stream"] = stream.numpy().astype(np.int16)
        out[f"{name}_oneshot"] = oneshot.numpy().astype(np.int16)
        out[f"{name}_margin"] = margin.numpy().astype(np.float32)
        meta["cases"][name] = {"cfg": cfg_name, "weights_seed": seed, "B": int(sig.shape[0]), "frames": frames, "pushes": sched,
                               "stream_vs_oneshot_differ": ndiff}
        print(f"{name}: B={sig.shape[0]} frames={frames} pushes={len(sched)}: streamed vs one-shot differ in {ndiff} tokens", flush=True)
    out["meta_json"] = np.frombuffer(json.dumps(meta, indent=1).encode(), dtype=np.uint8)
    path = os.path.join(GOLD, "mimi_stream_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
