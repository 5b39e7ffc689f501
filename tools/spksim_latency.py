#!/usr/bin/env python3
"""Time of the WavLM x-vector speaker similarity (audiocodecs_amd.spksim) against the same weights run the reference's way on the same GPU.

    python tools/spksim_latency.py [--least-calls 5 --window 2.0 --max-calls 50 --warmup 2] [--out profiles/spksim_latency.jsonl]

One process, one JSON line per shape: 32 pairs of 10 s and 1 pair of 3 s at 16 kHz (the metric's own rate: the resampler is timed by
tools of its own), seeded full-size weights (`checkpoint.synthetic_wavlm_sv_state_dict(WAVLM_BASE_SV)`).  The forms run on the SAME
signals on alternating calls, host clock from an idle device to an idle device:
    library    `SpeakerEncoder.embed_16k` of the 2 B clips and `cosine` of the two halves
    reference  downstream/metrics/speaker_similarity.py:101-120: transformers' `WavLMForXVector` in fp32 on the device (eager torch) and
               `torch.nn.functional.cosine_similarity`; where transformers is not importable, the statement of tests/spksim_ref.py in
               fp32 on the device (the same operations)
Also reported: the library's workspace for the shape, its kernels' share of a call (`profile_kernels`) and the largest difference of the
two forms' cosines.  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import SpeakerEncoder, checkpoint  # noqa: E402
from audiocodecs_amd.spksim import WAVLM_BASE_SV, cosine  # noqa: E402
from latency_common import alternate_for, emit, median_p99, shader_mhz  # noqa: E402

SHAPES = [("32 pairs x 10 s", 32, 160000), ("1 pair x 3 s", 1, 48000)]


def reference_form(cfg, sd):
    """(name, callable sig [2 B, L] -> cosines [B]) of the reference's way on the device."""
    try:
        import transformers

        model = transformers.WavLMForXVector(transformers.WavLMConfig(**cfg.hf_kwargs())).eval()
        model.load_state_dict(sd, strict=True)
        model = model.cuda()

        def run(sig):
            with torch.no_grad():
                e = model(input_values=sig, attention_mask=None, output_attentions=False).embeddings
            return torch.nn.functional.cosine_similarity(*e.split(len(e) // 2), dim=-1)

        return "transformers WavLMForXVector fp32", run
    except ImportError:
        import spksim_ref as R

        dev_sd = {k: v.cuda() for k, v in sd.items()}

        def run(sig):
            e = R.forward(cfg, dev_sd, sig, None, torch.float32)["emb"]
            return torch.nn.functional.cosine_similarity(*e.split(len(e) // 2), dim=-1)

        return "tests/spksim_ref.py fp32", run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--least-calls", type=int, default=5)
    ap.add_argument("--window", type=float, default=2.0)
    ap.add_argument("--max-calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import spksim_ref as R

    cfg = WAVLM_BASE_SV
    sd = checkpoint.synthetic_wavlm_sv_state_dict(cfg, 0)
    enc = SpeakerEncoder(state_dict=sd, arch=cfg)
    ref_name, ref = reference_form(cfg, sd)
    for name, pairs, L in SHAPES:
        sig = R.clips(2 * pairs, L, seed=pairs).cuda()

        def library():
            e = enc.embed_16k(sig)
            return cosine(e[:pairs], e[pairs:])

        forms = {"library": library, "reference": lambda: ref(sig)}
        lat, last, calls = alternate_for(forms, a.least_calls, a.window, a.max_calls, a.warmup)
        mhz = shader_mhz()
        nat = enc._native_for(sig)
        kernels = sorted(enc.profile_kernels(library), key=lambda r: -r[2])
        total = sum(r[2] for r in kernels)
        emit({"what": "spksim", "shape": name, "clips": 2 * pairs, "samples_16k": L, "calls": calls, "reference": ref_name,
              **median_p99(lat["library"], prefix="library_"), **median_p99(lat["reference"], prefix="reference_"),
              "workspace_MiB": round(nat.lib.ac_spk_workspace_bytes(nat.h, 2 * pairs, L) / 2**20, 1),
              "max_cosine_diff": float((last["library"] - last["reference"]).abs().max()), "shader_mhz": mhz,
              "kernel_ms_sum": round(total, 3), "top_kernels": [(r[0], r[1], round(r[2], 3)) for r in kernels[:8]]}, a.out)


if __name__ == "__main__":
    main()
