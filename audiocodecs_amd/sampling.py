"""Fused token sampling and on-device nearest-code token resampling: the reference's chain of softmax, top-k or
top-p, multinomial and gather (audiocodecs/codec.py:121-180; downstream/models/llama3.py:944-996) as ONE launch of the HIP library
(``ac_sample_tokens``) for all rows, with no intermediate tensor and nothing read back.  There is no CPU fallback.

Every draw is addressed by a counter of the repository's PRNG (prng.py): row ``r`` of a call with ``(seed, offset)`` uses the words
``2 * (offset + r)`` (mask) and ``2 * (offset + r) + 1`` (draw) of the stream ``key_for(seed, "sample")``.  The same ``(seed, offset)``
gives the same tokens on every machine, rows ``[a:b]`` of a call are the call on those rows at ``offset + a``, and a caller who generates
step by step advances ``offset`` by the number of rows per step.  ``offset`` may be a one-element int64 tensor on the device, which a
captured graph reads at every replay.

``sample_tokens(logits, ...)`` draws one token per row of ``logits`` [..., C].  ``resample_tokens(toks, logits_table, p, ...)`` is
``Codec.resample`` on the device: element ``(b, n, k)`` of ``toks`` [B, N, K] is replaced, with probability ``p``, by a draw from row
``toks[b, n, k]`` of ``logits_table[k]`` ([K, C, C]); the rows that the mask does not select are never read.

Semantics (stated once in include/audiocodecs_amd.h): weights ``exp((l - max) / temp)``; entries ranked by value descending, ties by
ascending index; ``top_k`` keeps the ranks below k, ``top_p`` keeps a rank while the mass ranked before it is at most ``p`` of the whole
(so ``top_k=1`` and ``top_p=0`` are argmax with the lowest index on ties); the draw walks the kept entries in ascending index order.  A
row with a NaN or without a finite maximum gives -1.
"""

from __future__ import annotations

import torch

from . import _metric_host as _host
from . import _native
from . import prng

__all__ = ["sample_tokens", "resample_tokens", "sample_form", "MIN_VOCAB", "MAX_VOCAB"]

MIN_VOCAB = 2
MAX_VOCAB = 16384
STREAM = "sample"      # the PRNG stream of every draw: key_for(seed, STREAM)


def sample_form(vocab_size: int) -> int:
    """1 (one wave per row) or 2 (one workgroup per row): the form rows of `vocab_size` logits take (a pure function of it; no GPU)."""
    _check_vocab(vocab_size)
    form = _native.lib().ac_sample_form(vocab_size)
    _native.check(form, None, "ac_sample_form")
    return form


def _check_vocab(C) -> None:
    if isinstance(C, bool) or not isinstance(C, int) or not MIN_VOCAB <= C <= MAX_VOCAB:
        raise ValueError(f"the number of logits per row ({C!r}) must be in {MIN_VOCAB}..{MAX_VOCAB}")


def _check_cuts(C: int, temp, top_k, top_p):
    """(temp, top_k or 0, top_p or -1) as the library takes them."""
    if top_k is not None and top_p is not None:
        raise NotImplementedError      # (as the reference: one cut at a time)
    temp = float(temp)
    if not 0.0 < temp < float("inf"):
        raise ValueError(f"`temp` ({temp}) must be positive and finite")
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 1 <= top_k <= C:
            raise ValueError(f"`top_k` ({top_k!r}) must be an int in 1..{C}")
    if top_p is not None:
        top_p = float(top_p)
        if not 0.0 <= top_p <= 1.0:
            raise ValueError(f"`top_p` ({top_p}) must be in [0, 1]")
    return temp, 0 if top_k is None else top_k, -1.0 if top_p is None else top_p


def _check_offset(offset, device=None):
    """(host part, device tensor or None); with `device`, a tensor has to live there."""
    if torch.is_tensor(offset):
        if offset.numel() != 1 or offset.dtype != torch.int64 or (device is not None and offset.device != device):
            raise ValueError("`offset` as a tensor must hold one int64 on the device of the logits")
        return 0, offset
    if isinstance(offset, bool) or not isinstance(offset, int) or not 0 <= offset < 1 << 62:
        raise ValueError(f"`offset` ({offset!r}) must be an int in [0, 2^62) or a one-element int64 tensor")
    return offset, None


def _launch(logits, row_stride, row_index, R, C, cuts, seed, offset, mask_p, fallback, out):
    temp, top_k, top_p = cuts
    host_offset, dev_offset = _check_offset(offset, logits.device)
    key = int(prng.key_for(seed, STREAM))
    with torch.cuda.device(logits.device):
        rc = _native.lib().ac_sample_tokens(_native._ptr(logits), row_stride, _native._ptr(row_index), R, C, temp, top_k, top_p, key, host_offset,
                                            _native._ptr(dev_offset), mask_p, _native._ptr(fallback), _native._ptr(out), _native._stream())
    _native.check(rc, None, "ac_sample_tokens")


@torch.no_grad()
def sample_tokens(logits: torch.Tensor, temp=1.0, top_k=None, top_p=None, seed=0, offset=0) -> torch.Tensor:
    """logits [..., C] fp32 on the device -> one int64 token per row, [...]; row r in flat order is element `offset + r` of the stream of
    `seed`.  A 2-D `logits` whose rows lie `stride(0) >= C` apart is read in place."""
    if not torch.is_tensor(logits) or logits.dim() < 1 or logits.dtype != torch.float32:
        raise ValueError("`logits` must be a [..., C] fp32 tensor")
    C = int(logits.shape[-1])
    _check_vocab(C)
    cuts = _check_cuts(C, temp, top_k, top_p)
    _check_offset(offset)
    _host.need_cuda(logits.is_cuda, "sampling", "logits")
    lead = logits.shape[:-1]
    R = 1
    for n in lead:
        R *= int(n)
    out = torch.empty(lead, dtype=torch.int64, device=logits.device)
    if R == 0:
        return out
    if logits.dim() == 2 and logits.stride(1) == 1 and (R == 1 or logits.stride(0) >= C):
        row_stride = max(int(logits.stride(0)), C)
    else:
        logits, row_stride = logits.contiguous(), C
    _launch(logits, row_stride, None, R, C, cuts, seed, offset, -1.0, None, out)
    return out


@torch.no_grad()
def resample_tokens(toks: torch.Tensor, logits_table: torch.Tensor, p, temp=1.0, top_k=None, top_p=None, seed=0, offset=0) -> torch.Tensor:
    """toks [B, N, K] (ids in [0, C)), logits_table [K, C, C] fp32 -> toks with every element replaced, with probability `p`, by a draw from
    row `toks[b, n, k]` of `logits_table[k]`; element (b, n, k) in flat order is row `offset + e` of the stream of `seed`.  `p <= 0`
    returns `toks` itself."""
    if p <= 0.0:
        return toks
    if not torch.is_tensor(toks) or toks.dim() != 3 or toks.is_floating_point() or toks.is_complex() or toks.dtype == torch.bool:
        raise ValueError("`toks` must be a [B, N, K] tensor of an integer dtype")
    K = int(toks.shape[-1])
    if not torch.is_tensor(logits_table) or logits_table.dim() != 3 or logits_table.dtype != torch.float32 or logits_table.shape[0] != K \
            or logits_table.shape[1] != logits_table.shape[2]:
        raise ValueError(f"`logits_table` must be a [K, C, C] = [{K}, C, C] fp32 tensor")
    C = int(logits_table.shape[-1])
    _check_vocab(C)
    cuts = _check_cuts(C, temp, top_k, top_p)
    p = float(p)
    if not p <= 1.0:
        raise ValueError(f"`p` ({p}) must be at most 1")
    _check_offset(offset)
    _host.need_cuda(toks.is_cuda and logits_table.is_cuda, "sampling", "tokens and the table")
    if logits_table.device != toks.device:
        raise ValueError(f"`toks` is on {toks.device}, `logits_table` on {logits_table.device}")
    fallback = toks.detach().to(torch.int64).contiguous()
    R = fallback.numel()
    out = torch.empty_like(fallback)
    if R == 0:
        return out.to(toks.dtype)
    # row k C + tok of the table as [K C, C]; an id out of range reads the nearest row of its codebook, never past the table
    row_index = fallback.clamp(0, C - 1) + torch.arange(K, device=toks.device) * C
    _launch(logits_table.contiguous(), C, row_index, R, C, cuts, seed, offset, p, fallback, out)
    return out.to(toks.dtype)
