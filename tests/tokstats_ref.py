"""Host statements of the codebook utilisation metric (pure torch, CPU) that the token statistics tests compare against.

  ref32_*     the reference's arithmetic (downstream/metrics/codebook_util.py) restated: fp32 counts filled clip by clip, probabilities,
              entropy and both ratios in fp32 tensors, the plain Python sum over the codebooks, the fp32 round trip before `round(.., 2)`.
              It reproduces the recorded summaries of tests/golden/tokstats_ref.npz exactly.
  stats64     the per-codebook quantities (ids in use, entropy in bits, utilisation, normalised entropy) in fp64 from exact integer
              counts: what `audiocodecs_amd.codebook_stats` computes on the device.
  histogram   `torch.bincount` per codebook: the exact oracle of `audiocodecs_amd.token_histogram`.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "tokstats_ref.npz")


def histogram(toks, vocab_size, nvalid=None):
    """toks [B, N, K] integer tensor (ids inside [0, vocab_size)) -> int64 [K, vocab_size]; nvalid [B]: frames of clip b that count."""
    toks = torch.as_tensor(toks).to(torch.int64).cpu()
    B, N, K = toks.shape
    if nvalid is not None:
        keep = torch.arange(N)[None, :] < torch.as_tensor(nvalid).to(torch.int64).cpu()[:, None]
        rows = toks[keep]
    else:
        rows = toks.reshape(B * N, K)
    return torch.stack([torch.bincount(rows[:, k], minlength=vocab_size) for k in range(K)])


def ref32_counts(clips, num_codebooks, vocab_size):
    """The reference's state after appending `clips` (each [1, N, K]) one by one: K fp32 count vectors and the number of frames."""
    counts = [torch.zeros(vocab_size) for _ in range(num_codebooks)]
    total = 0
    for clip in clips:
        clip = torch.as_tensor(clip).to(torch.int64)
        assert clip.dim() == 3 and clip.shape[0] == 1
        for k in range(num_codebooks):
            counts[k] += torch.bincount(clip[0, :, k], minlength=vocab_size)          # fp32 += int64, as the reference's indexed add
        total += clip.shape[0] * clip.shape[1]
    return counts, total


def ref32_summary(counts, total, vocab_size):
    """{"codebook_util", "norm_entropy"} from fp32 counts, in the reference's types and order of operations."""
    utils, ents = [], []
    for c in counts:
        p = c / total
        used = p > 0
        pv = p[used]
        h = -(pv * pv.log2()).sum()
        n_used = used.sum()
        if n_used > 1:
            utils.append(n_used / vocab_size)
            ents.append(h / math.log2(n_used))
        else:
            utils.append(0)
            ents.append(0.0)
    util = sum(utils) / len(utils)
    ent = sum(ents) / len(ents)
    as32 = lambda v: torch.as_tensor(v, dtype=torch.float32).item()      # (the reference's torch.tensor(v).item(): one fp32 round trip)
    return {"codebook_util": round(100 * as32(util), 2), "norm_entropy": round(100 * as32(ent), 2)}


def stats64(counts, total=None):
    """int64 counts [K, C] (total: frames counted; default the sum of row 0) -> fp64 [K, 4] = (ids in use, entropy, utilisation,
    normalised entropy); zeros for total == 0."""
    counts = torch.as_tensor(counts).to(torch.int64).cpu()
    K, C = counts.shape
    total = int(counts[0].sum()) if total is None else int(total)
    out = torch.zeros(K, 4, dtype=torch.float64)
    if total == 0:
        return out
    for k in range(K):
        p = counts[k].to(torch.float64) / float(total)
        pv = p[p > 0]
        n_used = int(pv.numel())
        h = float(-(pv * pv.log2()).sum())
        out[k, 0] = n_used
        out[k, 1] = h
        if n_used > 1:
            out[k, 2] = n_used / C
            out[k, 3] = h / math.log2(n_used)
    return out


def summary64(counts, total=None):
    """The two summary figures from `stats64`: round(100 * mean over the codebooks, 2)."""
    s = stats64(counts, total)
    K = s.shape[0]
    return {"codebook_util": round(100 * float(s[:, 2].sum()) / K, 2), "norm_entropy": round(100 * float(s[:, 3].sum()) / K, 2)}


def load_fixture():
    """[(name, K, C, clips, summary)]: clips a list of int64 [1, N, K] tensors, summary the reference class's recorded result."""
    z = np.load(FIXTURE)
    sets = []
    for name in [str(n) for n in z["names"]]:
        K, C = (int(v) for v in z[f"{name}.shape"])
        toks = torch.from_numpy(z[f"{name}.toks"].astype(np.int64))
        clips, at = [], 0
        for n in z[f"{name}.lengths"]:
            clips.append(toks[None, at:at + int(n)])
            at += int(n)
        util, ent = (float(v) for v in z[f"{name}.summary"])
        sets.append((name, K, C, clips, {"codebook_util": util, "norm_entropy": ent}))
    return sets


def padded_batch(clips):
    """Clips of different lengths as one batch: (toks [B, Nmax, K] padded with id 0, relative lens [B] fp32, nvalid [B])."""
    nmax = max(c.shape[1] for c in clips)
    toks = torch.zeros(len(clips), nmax, clips[0].shape[2], dtype=torch.int64)
    for b, c in enumerate(clips):
        toks[b, :c.shape[1]] = c[0]
    nvalid = torch.tensor([c.shape[1] for c in clips])
    return toks, (nvalid.to(torch.float64) / nmax).to(torch.float32), nvalid
