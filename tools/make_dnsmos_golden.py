#!/usr/bin/env python3
"""Writes the two DNSMOS fixtures under tests/golden/ (CPU only):

  dnsmos_p808.npz     the 16 tensors of the reference's P.808 model (downstream/metrics/model_v8.onnx) in fp32 under short names
                      (conv5.w .. conv9.b, dense3.w .. dense5.b).  The file is read with the package's own protobuf wire reader
                      (audiocodecs_amd.dnsmos.weights_from_onnx: onnx / onnxruntime are not needed), which refuses any graph whose node
                      list is not exactly the chain the package states.  The weights are data; nothing of the graph is written.
  dnsmos_golden.npz   values of OUR fp64 statement (tests/dnsmos_ref.py) -- not the reference's, whose librosa / onnxruntime are not on
                      disk: the six window scores of tests/golden/example.wav, every 30th frame of its first window's features, the
                      score of that window under white noise at 20, 5 and -5 dB SNR and of the noise alone (a MOS predictor must fall
                      with the SNR: the sanity anchor of the statement), and one window's score per synthetic signal kind.

Usage: tools/make_dnsmos_golden.py [--onnx PATH] [--out DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ANCHOR_SNRS = (20.0, 5.0, -5.0)
FEATURE_ROWS = np.arange(0, 900, 30)


def noisy(clean, snr_db, seed=0):
    """clean + white noise at `snr_db` (None: the noise alone, at the clean signal's power), fp32."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(len(clean))
    p = float(np.mean(clean.astype(np.float64) ** 2))
    n *= np.sqrt(p / np.mean(n ** 2))
    if snr_db is None:
        return n.astype(np.float32)
    return (clean.astype(np.float64) + n * 10.0 ** (-snr_db / 20.0)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--onnx", default="/root/reference/downstream/metrics/model_v8.onnx")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()

    from audiocodecs_amd.dnsmos import WEIGHT_SHAPES, weights_from_onnx

    with open(args.onnx, "rb") as f:
        w = weights_from_onnx(f.read())
    path = os.path.join(args.out, "dnsmos_p808.npz")
    np.savez(path, **{k: w[k].astype(np.float32) for k in WEIGHT_SHAPES})
    print(f"wrote {path}: {sum(v.size for v in w.values())} weights, {os.path.getsize(path)} bytes")

    import dnsmos_ref as R

    R.weights.cache_clear()
    x, rate = R.read_example()
    assert rate == R.FS
    mean, seg, feats = R.score_clip(x)
    out = {"example_scores": seg.astype(np.float64), "example_mean": np.float64(mean), "example_feature_rows": FEATURE_ROWS,
           "example_features": feats[0][FEATURE_ROWS].astype(np.float64)}
    first = x[:R.WINDOW]
    anchors = [float(R.net(R.features(noisy(first, s))[None])[0]) for s in ANCHOR_SNRS] + [float(R.net(R.features(noisy(first, None))[None])[0])]
    out["anchor_snrs"] = np.array(ANCHOR_SNRS)
    out["anchor_scores"] = np.array(anchors)
    for kind in R.KINDS:
        sig = R.make_signal(kind, R.WINDOW)
        out[f"{kind}_score"] = np.float64(R.net(R.features(sig)[None])[0])
    path = os.path.join(args.out, "dnsmos_golden.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    print("example windows:", np.round(seg, 4), "mean", round(mean, 4))
    print("anchors (20, 5, -5 dB, noise alone):", np.round(anchors, 3))
    print({k: round(float(out[f'{k}_score']), 4) for k in R.KINDS})


if __name__ == "__main__":
    main()
