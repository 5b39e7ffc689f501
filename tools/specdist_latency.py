#!/usr/bin/env python3
"""Call latency of `spectral_distances` against a torch restatement of the reference's two metric classes, on one GPU.

    python tools/specdist_latency.py [--calls 100 --warmup 5] [--out profiles/specdist_latency.jsonl]

One process; per shape (clips x seconds at 24 kHz, hypotheses P) in (64 x 10 s, 1), (64 x 10 s, 3), (1 x 10 s, 1) two forms run on the
SAME data on alternating calls (same clocks, same cache state):
    fused    `spectral_distances(hyp [P, B, T], ref, 24000)`: the library's resampler, then ac_specdist
    torch    downstream/metrics/stft_distance.py:49-69 and mel_distance.py:57-61 restated in torch on the same device, per hypothesis as
             the recipe appends them: the library's resampler (torchaudio is not installed), torch.stft, abs, the mel matmul, two log10
             passes per metric, subtraction, norm, mean.  The STFT is computed once per signal and shared by the two metrics, which the
             reference's two classes do not do: the restatement is the faster reading of the recipe.
Every call is timed on the host from the call to a stream synchronisation.  One JSON line per shape: median / p99 (ms) of each form,
the largest relative difference of the two results and the shader clock sampled while calls are queued (None where the platform
reports none).  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import spectral_distances  # noqa: E402
from audiocodecs_amd.resample import resample  # noqa: E402
from latency_common import alternate_for, emit, median_p99, shader_mhz  # noqa: E402

SHAPES = ((64, 10, 1), (64, 10, 3), (1, 10, 1))
RATE = 24000


def torch_restatement(hyp, ref, fb, win):
    def db(x):
        return 10.0 * torch.log10(torch.clamp(x, min=1e-10))

    def spec(x):
        m = torch.stft(resample(x, RATE, 16000), n_fft=1024, hop_length=320, window=win, return_complex=True).abs()
        return db(m), db(torch.matmul(m.transpose(-1, -2), fb).transpose(-1, -2))

    rs, rm = spec(ref)
    out = []
    for p in range(hyp.shape[0]):
        hs, hm = spec(hyp[p])
        out.append(((hs - rs).norm(dim=1).mean(dim=1), (hm - rm).norm(dim=1).mean(dim=1)))
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


def main():
    import specdist_ref as R

    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100, help="least number of timed calls per form and shape")
    ap.add_argument("--window", type=float, default=1.0, help="least timed seconds of the fastest form per shape")
    ap.add_argument("--max-calls", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    fb = torch.from_numpy(R.filterbank()).float().cuda()
    win = torch.hann_window(1024, device="cuda")
    for B, secs, P in SHAPES:
        g = torch.Generator().manual_seed(B + P)
        T = secs * RATE
        ref = (0.1 * torch.randn(B, T, generator=g)).cuda()
        hyp = ref[None] + (0.01 * torch.randn(P, B, T, generator=g)).cuda()
        forms = {
            "fused": lambda: spectral_distances(hyp, ref, RATE),
            "torch": lambda: torch_restatement(hyp, ref, fb, win),
        }
        lat, last, calls = alternate_for(forms, a.calls, a.window, a.max_calls, a.warmup)
        assert all(out[0].shape == (P, B) for out in last.values())
        row = {"clips": B, "seconds": secs, "rate": RATE, "P": P, "frames": 1 + (secs * 16000) // 320, "calls": calls, "warmup": a.warmup}
        for name, v in lat.items():
            row.update(median_p99(v, prefix=f"{name}_"))
        for _ in range(20):
            spectral_distances(hyp, ref, RATE)
        row["shader_mhz"] = shader_mhz()
        torch.cuda.synchronize()
        fs, fm = spectral_distances(hyp, ref, RATE)
        ts, tm = torch_restatement(hyp, ref, fb, win)
        row["largest_relative_difference"] = float(max(((fs - ts).abs() / ts.abs()).max(), ((fm - tm).abs() / tm.abs()).max()))
        emit(row, a.out)


if __name__ == "__main__":
    main()
