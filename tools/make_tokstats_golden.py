#!/usr/bin/env python3
"""Writes tests/golden/tokstats_ref.npz (CPU only): seeded token sets and what the REFERENCE's own `CodebookUtil` class
(downstream/metrics/codebook_util.py) returns for them, appended clip by clip at B = 1 as the class demands.

The class derives from speechbrain's `MetricStats`, which is not needed for what it computes and may not be installed: when the import
fails, an empty stand-in class of that name is registered for the import.  Nothing of the reference's text is written: per set the
fixture holds `<name>.shape` = (K, C), `<name>.toks` int16 [sum of N, K] (the clips one after another), `<name>.lengths` and
`<name>.summary` = (codebook_util, norm_entropy), the two rounded figures the class returned.

Sets: uniform ids; Zipf-like ids (weight 1 / rank, a seeded permutation of the ranks per codebook); one id only; two ids; a mixture whose
codebooks differ in kind -- over K in {1, 8, 9} and C in {512, 1024, 2048}.

Usage: tools/make_tokstats_golden.py [--reference DIR] [--out DIR]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# (name, kind, K, C, clip lengths)
SETS = [
    ("uniform_k8_c1024", "uniform", 8, 1024, (75, 113, 150)),
    ("uniform_k9_c512", "uniform", 9, 512, (61, 97, 128)),
    ("uniform_k1_c2048", "uniform", 1, 2048, (300, 211, 450)),
    ("zipf_k8_c2048", "zipf", 8, 2048, (125, 90, 140)),
    ("zipf_k1_c512", "zipf", 1, 512, (200, 333)),
    ("zipf_k9_c1024", "zipf", 9, 1024, (80, 121, 64)),
    ("onebin_k8_c1024", "onebin", 8, 1024, (40, 57)),
    ("twobins_k1_c512", "twobins", 1, 512, (33, 64, 18)),
    ("mixed_k9_c2048", "mixed", 9, 2048, (100, 77, 131)),
]
KINDS = ("uniform", "zipf", "onebin", "twobins")


def column(kind, C, n, rng):
    """n ids of one codebook."""
    if kind == "uniform":
        return rng.integers(0, C, n)
    if kind == "zipf":
        w = 1.0 / np.arange(1, C + 1)
        return rng.permutation(C)[rng.choice(C, size=n, p=w / w.sum())]
    if kind == "onebin":
        return np.full(n, rng.integers(0, C))
    if kind == "twobins":
        return rng.choice(rng.choice(C, size=2, replace=False), size=n)
    raise ValueError(kind)


def make_set(index, kind, K, C, lengths):
    """The clips of a set, each int64 [1, N, K]; codebook k of a mixed set is of kind k % 4."""
    rng = np.random.default_rng(20250 + index)
    total = sum(lengths)
    cols = [column(KINDS[k % 4] if kind == "mixed" else kind, C, total, rng) for k in range(K)]
    toks = np.stack(cols, axis=1).astype(np.int64)
    clips, at = [], 0
    for n in lengths:
        clips.append(torch.from_numpy(toks[None, at:at + n]))
        at += n
    return toks, clips


def reference_class(reference):
    try:
        import speechbrain.utils.metric_stats  # noqa: F401
    except ImportError:
        for name in ("speechbrain", "speechbrain.utils", "speechbrain.utils.metric_stats"):
            sys.modules.setdefault(name, types.ModuleType(name))
        sys.modules["speechbrain.utils.metric_stats"].MetricStats = type("MetricStats", (), {"clear": lambda self: None})
    spec = importlib.util.spec_from_file_location("reference_codebook_util", os.path.join(reference, "downstream", "metrics", "codebook_util.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.CodebookUtil


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    args = ap.parse_args()
    CodebookUtil = reference_class(args.reference)

    out = {"names": np.array([s[0] for s in SETS])}
    for index, (name, kind, K, C, lengths) in enumerate(SETS):
        toks, clips = make_set(index, kind, K, C, lengths)
        metric = CodebookUtil(K, C)
        for clip in clips:
            metric.append(clip)
        summary = metric.summarize()
        out[f"{name}.shape"] = np.array([K, C], dtype=np.int32)
        out[f"{name}.toks"] = toks.astype(np.int16)
        out[f"{name}.lengths"] = np.array(lengths, dtype=np.int32)
        out[f"{name}.summary"] = np.array([summary["codebook_util"], summary["norm_entropy"]], dtype=np.float64)
        print(f"{name}: {summary}")
    path = os.path.join(args.out, "tokstats_ref.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
