"""Token histograms and codebook utilisation: the one metric of the reference's resynthesis recipe that reads the TOKENS
(the reference's downstream/metrics/codebook_util.py; downstream/test_sr.py:103-112), on the device the encode left them on.

``token_histogram(toks, vocab_size)`` counts, per codebook, how often every id occurs in ``toks`` [B, N, K]: one launch of the HIP library
(``ac_tokstats_accumulate``), exact int64 counts, nothing read back.  ``codebook_stats`` turns counts into the
reference's per-codebook quantities in fp64 (``ac_tokstats_summary``): the number of ids in use, the entropy in bits, the utilisation and the
normalised entropy.  There is no CPU fallback.

``CodebookUtil`` has the reference class's constructor, ``append``, ``summarize`` and ``clear``.  It differs from it in four ways:
  * ``append`` takes any batch size (the reference asserts B == 1) and makes no host copy (the reference makes 2 K per clip);
  * counts are int64 (the reference's are fp32, which stops being exact at 2^24 occurrences of one id);
  * ``lens`` is honoured: it is relative, as everywhere in this API, and clip b contributes its first
    ``clamp(round(lens[b] * N), 0, N)`` frames (``torch.round``: halves go to the even neighbour).  **The reference ignores ``lens`` here**
    and counts the padding of a batch; with B == 1 and ``lens`` of None or 1 the two agree exactly;
  * an id outside [0, vocab_size) is never counted and never an index; ``summarize`` raises ``ValueError`` when any was met, where the
    reference raises ``IndexError`` at the ``append``.
``summarize`` is the one place that reads the device: one copy of K * 4 + 1 numbers.
"""

from __future__ import annotations

import torch

from . import _metric_host as _host
from . import _native

__all__ = ["token_histogram", "codebook_stats", "tokstats_form", "TokenStatsState", "CodebookUtil", "MAX_CODEBOOKS", "MIN_VOCAB", "MAX_VOCAB"]

MAX_CODEBOOKS = 64
MIN_VOCAB = 2
MAX_VOCAB = 1 << 20


def _check_shape(num_codebooks, vocab_size) -> None:
    for name, v in (("num_codebooks", num_codebooks), ("vocab_size", vocab_size)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"`{name}` ({v!r}) must be an int")
    if not 1 <= num_codebooks <= MAX_CODEBOOKS:
        raise ValueError(f"`num_codebooks` ({num_codebooks}) must be in 1..{MAX_CODEBOOKS}")
    if not MIN_VOCAB <= vocab_size <= MAX_VOCAB:
        raise ValueError(f"`vocab_size` ({vocab_size}) must be in {MIN_VOCAB}..{MAX_VOCAB}")


def tokstats_form(num_codebooks: int, vocab_size: int):
    """("tiled", G) or ("direct", 0): the form a histogram of this shape takes (a pure function of the two; no GPU)."""
    _check_shape(num_codebooks, vocab_size)
    G = _native.lib().ac_tokstats_form(num_codebooks, vocab_size)
    _native.check(G, None, "ac_tokstats_form")
    return ("tiled", G) if G > 0 else ("direct", 0)


class TokenStatsState:
    """The device state the kernels add into: ONE int64 buffer ``buf`` of K * C + 2 words -- ``counts`` [K, C], ``total`` (frames counted),
    ``bad`` (ids outside [0, C) among them); the three attributes are views of it."""

    def __init__(self, num_codebooks: int, vocab_size: int, device):
        _check_shape(num_codebooks, vocab_size)
        device = torch.device(device)
        _host.need_cuda(device.type == "cuda", "tokstats", "state", "the {} lives on")
        self.num_codebooks, self.vocab_size = num_codebooks, vocab_size
        self.buf = torch.zeros(num_codebooks * vocab_size + 2, dtype=torch.int64, device=device)

    @property
    def counts(self) -> torch.Tensor:
        return self.buf[:-2].view(self.num_codebooks, self.vocab_size)

    @property
    def total(self) -> torch.Tensor:
        return self.buf[-2]

    @property
    def bad(self) -> torch.Tensor:
        return self.buf[-1]

    def clear(self) -> None:
        self.buf.zero_()


def _nvalid(lens, B: int, N: int, device) -> torch.Tensor:
    """clamp(round(lens * N), 0, N) as int32 [B] on the device, without a synchronisation."""
    lens = torch.as_tensor(lens)
    if lens.dim() != 1 or lens.shape[0] != B:
        raise ValueError(f"`lens` must be [B] = [{B}] (got {tuple(lens.shape)})")
    return (lens.to(device=device, dtype=torch.float64) * N).round().clamp(0, N).to(torch.int32)


@torch.no_grad()
def token_histogram(toks: torch.Tensor, vocab_size: int, lens=None, out=None) -> torch.Tensor:
    """toks [B, N, K] (any integer dtype) -> counts [K, vocab_size] int64 on the tokens' device.  `lens` [B], relative: clip b contributes
    its first clamp(round(lens[b] * N), 0, N) frames.  `out` accumulates: a `TokenStatsState` (its `total` and `bad` are kept too) or an
    int64 [K, vocab_size] tensor of counts; the counts are returned either way.  Ids outside [0, vocab_size) are not counted."""
    if not torch.is_tensor(toks) or toks.dim() != 3 or toks.is_floating_point() or toks.is_complex() or toks.dtype == torch.bool:
        raise ValueError("`toks` must be a [B, N, K] tensor of an integer dtype")
    B, N, K = (int(n) for n in toks.shape)
    _check_shape(K, vocab_size)
    _host.need_cuda(toks.is_cuda, "tokstats", "tokens")
    dev = toks.device
    state = out if isinstance(out, TokenStatsState) else TokenStatsState(K, vocab_size, dev)
    if (state.num_codebooks, state.vocab_size) != (K, vocab_size) or state.buf.device != dev:
        raise ValueError(f"`out` holds {state.num_codebooks} codebooks of {state.vocab_size} on {state.buf.device}; "
                         f"the tokens have {K} of {vocab_size} on {dev}")
    if out is not None and state is not out:
        if not torch.is_tensor(out) or out.dtype != torch.int64 or tuple(out.shape) != (K, vocab_size) or out.device != dev:
            raise ValueError(f"`out` must be a TokenStatsState or an int64 [{K}, {vocab_size}] tensor on {dev}")
    nvalid = None if lens is None else _nvalid(lens, B, N, dev)
    toks = toks.detach().to(torch.int64).contiguous()
    L = _native.lib()
    with torch.cuda.device(dev):
        rc = L.ac_tokstats_accumulate(_native._ptr(toks), B, N, K, vocab_size, _native._ptr(nvalid), _native._ptr(state.buf),
                                      state.buf.numel() * 8, _native._stream())
    _native.check(rc, None, "ac_tokstats_accumulate")
    if out is not None and state is not out:
        out += state.counts
        return out
    return state.counts


@torch.no_grad()
def codebook_stats(counts_or_state) -> torch.Tensor:
    """A `TokenStatsState`, or int64 counts [K, C] whose rows each sum to the number of frames -> [K, 4] fp64 on the same device:
    per codebook (ids in use, entropy in bits, utilisation, normalised entropy); the last two are 0 unless two ids are in use."""
    state = counts_or_state
    if not isinstance(state, TokenStatsState):
        counts = counts_or_state
        if not torch.is_tensor(counts) or counts.dim() != 2 or counts.dtype != torch.int64:
            raise ValueError("`counts_or_state` must be a TokenStatsState or an int64 [K, C] tensor")
        state = TokenStatsState(int(counts.shape[0]), int(counts.shape[1]), counts.device)
        state.counts.copy_(counts)
        state.total.copy_(counts[0].sum())
    K, Cv = state.num_codebooks, state.vocab_size
    out = torch.empty(K, 4, dtype=torch.float64, device=state.buf.device)
    L = _native.lib()
    with torch.cuda.device(state.buf.device):
        rc = L.ac_tokstats_summary(_native._ptr(state.buf), K, Cv, _native._ptr(out), _native._stream())
    _native.check(rc, None, "ac_tokstats_summary")
    return out


class CodebookUtil:
    """downstream/metrics/codebook_util.py: the share of every codebook's ids that the appended tokens use and the entropy of their
    distribution over the ids in use, each averaged over the codebooks.  The module's docstring lists what differs from the reference
    (any batch size, int64 counts, `lens` honoured, ids out of range).  Of speechbrain's ``MetricStats`` only ``append``, ``summarize``
    and ``clear`` exist."""

    def __init__(self, num_codebooks, vocab_size):
        _check_shape(num_codebooks, vocab_size)
        self.num_codebooks = num_codebooks
        self.vocab_size = vocab_size
        self.state = None          # created on the device of the first tokens
        self.clear()

    def clear(self) -> None:
        if self.state is not None:
            self.state.clear()
        self.summary = {}

    @torch.no_grad()
    def append(self, hyp_toks, lens=None) -> None:
        """hyp_toks [B, N, K]; `lens` [B] relative or None.  No host copy, no synchronisation."""
        if not torch.is_tensor(hyp_toks) or hyp_toks.dim() != 3 or hyp_toks.shape[-1] != self.num_codebooks:
            raise ValueError(f"`hyp_toks` must be [B, N, {self.num_codebooks}]")
        _host.need_cuda(hyp_toks.is_cuda, "tokstats", "tokens")
        if self.state is None:
            self.state = TokenStatsState(self.num_codebooks, self.vocab_size, hyp_toks.device)
        token_histogram(hyp_toks, self.vocab_size, lens=lens, out=self.state)

    def summarize(self, field=None):
        """{"codebook_util", "norm_entropy"}: round(100 * mean over the codebooks, 2).  Nothing appended gives 0 and 0, as the reference does."""
        util = entropy = 0.0
        if self.state is not None:
            host = torch.cat([codebook_stats(self.state).flatten(), self.state.bad.to(torch.float64)[None]]).cpu()      # the one read
            if host[-1] != 0:
                raise ValueError(f"{int(host[-1])} token ids outside [0, {self.vocab_size}) were appended")
            per = host[:-1].view(self.num_codebooks, 4)
            util = float(per[:, 2].sum()) / self.num_codebooks
            entropy = float(per[:, 3].sum()) / self.num_codebooks
        self.summary = {"codebook_util": round(100 * util, 2), "norm_entropy": round(100 * entropy, 2)}
        return self.summary if field is None else self.summary[field]
