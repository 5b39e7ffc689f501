"""Cosine k-nearest-neighbour feature matching: the single-codebook voice-conversion step of the reference's evaluation recipe
(/root/reference/downstream/test_vc.py:116-128: ``knn(hyp_feats, matching_set, topk, num_splits).mean(dim=-2)``) as one call.

``knn_match(feats, matching_set)`` returns, for every feature row, the mean of the ``topk`` rows of the matching set with the largest
cosine similarity.  It runs in the HIP library (``ac_knn_pack`` / ``ac_knn_match``): no [Q, M] distance matrix,
no top-k pass, no [Q, k, H] gather; there is no CPU fallback.  ``KnnIndex`` holds a matching set with its packed image so that one
target speaker is packed once and matched many times.  ``knn`` has the reference helper's signature and result ([..., k, H], nearest
first) for callers that want the neighbours themselves.

Two stated departures from the reference helper.  Both sides are L2-normalised first and the similarity is one dot product of unit
vectors, where the reference rebuilds the dot product from ``|q|^2 + |t|^2 - cdist^2`` and cancels in fp32 (DESIGN.md has the figures).
And rows without a direction -- a zero row, a row of denormals, a row with an inf or a NaN -- never match and are never matched: such a
matching row is skipped, such a query row gets a NaN output row and indices -1, and neither disturbs any other row (the reference
yields NaN distances and arbitrary picks).  Equal computed similarities go to the lower index.
"""

from __future__ import annotations

import torch

from . import _metric_host as _host
from . import _native

__all__ = ["knn_match", "knn", "KnnIndex", "auto_splits", "WIDTHS", "MAX_TOPK"]

WIDTHS = (32, 64, 128, 256, 512)     # the compiled feature widths; a narrower multiple of 32 is zero-padded to the next (zeros leave the cosine alone)
MAX_TOPK = 8
MAX_SPLITS = 64


def _padded_width(H: int) -> int:
    if H < 1 or H % 32 or H > WIDTHS[-1]:
        raise ValueError(f"feature width ({H}) must be a multiple of 32 up to {WIDTHS[-1]}")
    return next(w for w in WIDTHS if w >= H)


def _check_topk(topk) -> int:
    if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= MAX_TOPK:
        raise ValueError(f"`topk` ({topk!r}) must be an int in 1..{MAX_TOPK}")
    return topk


def _check_splits(num_splits) -> int:
    if num_splits is None:
        return 0
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or not 1 <= num_splits <= MAX_SPLITS:
        raise ValueError(f"`num_splits` ({num_splits!r}) must be None (chosen from the shapes) or an int in 1..{MAX_SPLITS}")
    return num_splits


def auto_splits(Q: int, M: int, H: int) -> int:
    """The number of slices of the matching set a match of Q rows against M rows of width H walks side by side when the caller names
    none (``ac_knn_num_splits``: pure host arithmetic, needs no GPU)."""
    s = _native.lib().ac_knn_num_splits(int(Q), int(M), _padded_width(int(H)), 0)
    if s < 1:
        raise ValueError(f"auto_splits: bad arguments (Q={Q}, M={M}, H={H})")
    return int(s)


class KnnIndex:
    """A matching set [M, H] on a cuda device with its packed image (L2-normalised rows as split16 planes in the match kernel's tile
    order): build once per target speaker, ``match`` any number of utterances against it."""

    def __init__(self, matching_set: torch.Tensor):
        if not torch.is_tensor(matching_set) or matching_set.dim() != 2:
            raise ValueError("`matching_set` must be a [M, H] tensor")
        M, H = matching_set.shape
        if M < 1:
            raise ValueError("`matching_set` is empty (M = 0): there is nothing to match")
        self.width = int(H)
        self._Hp = _padded_width(self.width)
        _host.need_cuda(matching_set.is_cuda, "knn", "matching set")
        self.device = matching_set.device
        s = matching_set.detach().to(torch.float32)
        if self._Hp != self.width:
            s = torch.nn.functional.pad(s, (0, self._Hp - self.width))
        self.set = s.contiguous()                    # the fp32 rows that are averaged (zero-padded to the compiled width)
        self.rows = int(M)
        self._lib = _native.lib()
        self.packed = _host.sized_buffer("ac_knn_packed_bytes", self.device, M=self.rows, H=self._Hp)
        with torch.cuda.device(self.device):
            rc = self._lib.ac_knn_pack(_native._ptr(self.set), self.rows, self._Hp, _native._ptr(self.packed), self.packed.numel(), _native._stream())
        _native.check(rc, None, "ac_knn_pack")

    def match(self, feats: torch.Tensor, topk: int = 4, num_splits=None, return_indices: bool = False):
        """feats [..., H] -> [..., H]: per row the mean of its k = min(topk, valid rows) nearest rows.  With `return_indices` also the
        indices [..., topk] (int64, nearest first, -1 behind k) and cosine similarities [..., topk] (fp32, NaN behind k)."""
        topk, S = _check_topk(topk), _check_splits(num_splits)
        if not torch.is_tensor(feats) or feats.dim() < 1 or feats.shape[-1] != self.width:
            raise ValueError(f"`feats` must be [..., {self.width}] like the matching set (got {tuple(feats.shape) if torch.is_tensor(feats) else type(feats)})")
        _host.need_cuda(feats.is_cuda, "knn", "features")
        if feats.device != self.device:
            raise ValueError(f"`feats` is on {feats.device}, the matching set on {self.device}")
        lead = tuple(feats.shape[:-1])
        Q = 1
        for n in lead:
            Q *= int(n)
        if Q == 0:     # nothing to match: the empty result (the library is not called)
            out = torch.empty(lead + (self.width,), dtype=torch.float32, device=self.device)
            if return_indices:
                return out, torch.empty(lead + (topk,), dtype=torch.int64, device=self.device), torch.empty(lead + (topk,), dtype=torch.float32, device=self.device)
            return out
        q = feats.detach().to(torch.float32).reshape(Q, self.width)
        if self._Hp != self.width:
            q = torch.nn.functional.pad(q, (0, self._Hp - self.width))
        q = q.contiguous()
        out = torch.empty(Q, self._Hp, dtype=torch.float32, device=self.device)
        idx = torch.empty(Q, topk, dtype=torch.int64, device=self.device) if return_indices else None
        sim = torch.empty(Q, topk, dtype=torch.float32, device=self.device) if return_indices else None
        ws = _host.sized_buffer("ac_knn_workspace_bytes", self.device, Q=Q, M=self.rows, H=self._Hp, topk=topk, num_splits=S)
        ptr = _native._ptr
        with torch.cuda.device(self.device):
            rc = self._lib.ac_knn_match(ptr(q), Q, ptr(self.set), ptr(self.packed), self.rows, self._Hp, topk, S, ptr(out), ptr(idx), ptr(sim), ptr(ws), ws.numel(),
                                        _native._stream())
        _native.check(rc, None, "ac_knn_match")
        out = out[:, :self.width].reshape(lead + (self.width,))
        if return_indices:
            return out, idx.reshape(lead + (topk,)), sim.reshape(lead + (topk,))
        return out


def _index_for(feats, matching_set) -> KnnIndex:
    """Host-side argument checks that need both sides, before any device call; packs a plain tensor."""
    if isinstance(matching_set, KnnIndex):
        return matching_set
    if not torch.is_tensor(matching_set) or matching_set.dim() != 2:
        raise ValueError("`matching_set` must be a [M, H] tensor or a KnnIndex")
    if matching_set.shape[0] < 1:
        raise ValueError("`matching_set` is empty (M = 0): there is nothing to match")
    if torch.is_tensor(feats):
        if feats.dim() < 1 or feats.shape[-1] != matching_set.shape[-1]:
            raise ValueError(f"width mismatch: `feats` {tuple(feats.shape)} against `matching_set` {tuple(matching_set.shape)}")
        if feats.is_cuda and matching_set.is_cuda and feats.device != matching_set.device:
            raise ValueError(f"`feats` is on {feats.device}, the matching set on {matching_set.device}")
    _padded_width(int(matching_set.shape[-1]))
    return KnnIndex(matching_set)


def knn_match(feats: torch.Tensor, matching_set, topk: int = 4, num_splits=None, return_indices: bool = False):
    """feats [..., H], matching_set [M, H] (or a `KnnIndex`) -> [..., H]: per row the mean of its `topk` nearest rows of the set by
    cosine similarity -- ``knn(feats, matching_set, topk).mean(dim=-2)`` of the reference recipe in one call.  `num_splits`: None lets the
    library choose how many slices of the set it walks side by side; any value returns the same bits."""
    _check_topk(topk)
    _check_splits(num_splits)
    return _index_for(feats, matching_set).match(feats, topk, num_splits, return_indices)


def knn(input: torch.Tensor, matching_set, topk: int = 4, num_splits: int = 1):
    """The reference helper's signature and result (downstream/test_vc.py:359): input [..., H] -> the neighbours [..., k, H], nearest
    first, k = min(topk, rows that can be matched), gathered from the set by the matched indices."""
    _check_topk(topk)
    _check_splits(num_splits)
    index = _index_for(input, matching_set)
    _, idx, _ = index.match(input, topk, num_splits, return_indices=True)
    k = int((idx >= 0).sum(dim=-1).max()) if idx.numel() else min(topk, index.rows)
    idx = idx[..., :k]
    out = index.set[:, :index.width][idx.clamp_min(0)]
    return out.masked_fill((idx < 0)[..., None], float("nan"))     # (a query row without a direction has no neighbours)
