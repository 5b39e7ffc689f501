#!/usr/bin/env python3
"""Generate tests/golden/specdist_golden.npz: fp64 spectral distances from torch.stft.

    python tools/make_specdist_golden.py

The fixture pins tests/specdist_ref.py (the project's fp64 statement of the two distances: explicit framing and numpy's rfft) to what the
reference calls.  Per case it holds the seed and shape of a signal pair (tests/specdist_ref.py make_pair rebuilds the samples) and the
scores of the reference's downstream/metrics/stft_distance.py:49-69 restated on ``torch.stft`` in fp64: magnitude, AmplitudeToDB's
default rule, L2 norm over bins, mean over frames.  The mel scores apply torchaudio's HTK filterbank formula, written out here in torch
ops, to the same magnitudes (mel_distance.py:57-61); torchaudio itself is not installed, so that part is a restatement on both sides.
Data only: seeds, shapes, scores.
"""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import specdist_ref as R  # noqa: E402  (signal makers only)

CASES = [(kind, 100 + 10 * i + j, 2, L) for i, kind in enumerate(R.KINDS) for j, L in enumerate((513, 5121, 16000))]


def amplitude_to_db(x):
    return 10.0 * torch.log10(torch.clamp(x, min=1e-10))


def melscale_fbanks():
    all_freqs = torch.linspace(0, 8000, 513, dtype=torch.float64)
    m_max = 2595.0 * math.log10(1.0 + 8000.0 / 700.0)
    m_pts = torch.linspace(0.0, m_max, 82, dtype=torch.float64)
    f_pts = 700.0 * (10 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down_slopes = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up_slopes = slopes[:, 2:] / f_diff[1:]
    return torch.max(torch.zeros(1, dtype=torch.float64), torch.min(down_slopes, up_slopes))


def scores(hyp, ref):
    win = torch.hann_window(1024, dtype=torch.float64)
    fb = melscale_fbanks()
    mag = [torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft=1024, hop_length=320, window=win, return_complex=True).abs() for x in (hyp, ref)]
    sf = (amplitude_to_db(mag[0]) - amplitude_to_db(mag[1])).norm(dim=1)
    mel = [torch.matmul(m.transpose(-1, -2), fb).transpose(-1, -2) for m in mag]
    mf = (amplitude_to_db(mel[0]) - amplitude_to_db(mel[1])).norm(dim=1)
    return sf.mean(dim=1).numpy(), mf.mean(dim=1).numpy(), sf.numpy(), mf.numpy()


def main():
    out, meta = {}, {"source": "torch.stft in fp64 + downstream/metrics/stft_distance.py:49-69, mel_distance.py:57-61 restated", "torch": torch.__version__, "cases": []}
    for c, (kind, seed, B, L) in enumerate(CASES):
        hyp, ref = R.make_pair(kind, seed, B, L)
        s, m, sf, mf = scores(hyp, ref)
        assert sf.shape == (B, 1 + L // 320)
        out[f"c{c}_stft"], out[f"c{c}_mel"], out[f"c{c}_stft_frames"], out[f"c{c}_mel_frames"] = s, m, sf, mf
        meta["cases"].append({"kind": kind, "seed": seed, "B": B, "L": L})
    out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "specdist_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    sys.exit(main())
