"""The downstream recipes' probe over codec tokens on the HIP library (csrc/probe_path.hip):

    toks [B, N, K] -> MultiHeadEmbedding -> LinearPooling | AttentionalPooling -> [B, N, E]
                   -> bidirectional LSTM over packed sequences (lengths) -> [B, N, 2 H]
                   -> "ctc":        Linear(2 H, num_classes) -> log_softmax -> CTC greedy decode
                      "utterance":  mean | std over the valid frames -> Linear(4 H, num_classes) -> log_softmax

Refused, with a message, before any launch: a list-valued `vocab_size` (per-codebook vocabularies), a `hidden_size` that is no multiple
of 32 (or has no recurrence kernel: 32, 64, 128, 256 and 512 are compiled), an input width that is no multiple of 32 (what the matrix
pipe packs) and exact-product arithmetic.  The thin speechbrain wrappers around the model (``RNN.LSTM``, ``StatisticsPooling``,
``ctc_greedy_decode``) are restated from their documentation, not pinned to that library; `StatisticsPooling`'s 1e-5-scale jitter on the
mean is not reproduced.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional

import torch

from . import _metric_host as _host
from . import _native

__all__ = ["ProbeConfig", "ProbeOutput", "TokenProbe", "PROBE_TINY", "PROBE_RECIPE", "fold_attn_scores", "weight_names", "relative_to_frames"]

POOLINGS = {None: 0, "linear": 1, "attentional": 2}
HEADS = {"ctc": 0, "utterance": 1}
HIDDEN_SIZES = (32, 64, 128, 256, 512)     # bilstm_step_kernel's instances
MAX_CODEBOOKS = 32


@dataclass(frozen=True)
class ProbeConfig:
    vocab_size: int = 1024
    num_codebooks: int = 2
    embedding_dim: int = 128
    hidden_size: int = 512
    num_layers: int = 2
    pooling: Optional[str] = "linear"      # None: the recipes' use_quantized_feats -- the input is [B, N, embedding_dim] floats
    head: str = "ctc"
    num_classes: int = 1001
    blank_id: int = 0
    padding_idx: bool = False

    @property
    def table_rows(self) -> int:
        return self.vocab_size * self.num_codebooks + (1 if self.padding_idx else 0)

    @property
    def head_in(self) -> int:
        return (2 if self.head == "ctc" else 4) * self.hidden_size


PROBE_TINY = ProbeConfig(vocab_size=50, num_codebooks=2, embedding_dim=32, hidden_size=64, num_layers=2, pooling="linear", head="ctc", num_classes=11)
PROBE_RECIPE = ProbeConfig()     # EnCodec tokens, the ASR recipe: K = 2, C = 1024, E = 128, H = 512, two layers, 1000 tokens + blank


def check_config(cfg: ProbeConfig) -> None:
    """Every refusal that needs no device."""
    if isinstance(cfg.vocab_size, (list, tuple)):
        raise NotImplementedError("a list-valued `vocab_size` (one vocabulary per codebook) is not compiled: the table's offsets are k * vocab_size")
    for name in ("vocab_size", "num_codebooks", "embedding_dim", "hidden_size", "num_layers", "num_classes", "blank_id"):
        v = getattr(cfg, name)
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"`{name}` ({v!r}) must be an int")
    if cfg.pooling not in POOLINGS:
        raise ValueError(f"`pooling` ({cfg.pooling!r}) must be one of {list(POOLINGS)}")
    if cfg.head not in HEADS:
        raise ValueError(f"`head` ({cfg.head!r}) must be one of {list(HEADS)}")
    if cfg.hidden_size < 32 or cfg.hidden_size % 32:
        raise ValueError(f"`hidden_size` ({cfg.hidden_size}) must be a multiple of 32: the recurrence walks K in halves of 16-wide MFMA steps")
    if cfg.hidden_size not in HIDDEN_SIZES:
        raise ValueError(f"`hidden_size` ({cfg.hidden_size}) has no recurrence kernel: {HIDDEN_SIZES} are compiled")
    if cfg.embedding_dim < 32 or cfg.embedding_dim % 32:
        raise ValueError(f"`embedding_dim` ({cfg.embedding_dim}), the input width of the first projection, must be a multiple of 32: what the matrix pipe packs")
    if not 1 <= cfg.num_layers <= 8:
        raise ValueError(f"`num_layers` ({cfg.num_layers}) must be in 1..8")
    if cfg.num_classes < 1:
        raise ValueError("`num_classes` must be positive")
    if cfg.pooling is not None and (not 1 <= cfg.num_codebooks <= MAX_CODEBOOKS or cfg.vocab_size < 1):
        raise ValueError(f"`num_codebooks` ({cfg.num_codebooks}) must be in 1..{MAX_CODEBOOKS} and `vocab_size` positive")
    if cfg.head == "ctc" and not 0 <= cfg.blank_id < cfg.num_classes:
        raise ValueError(f"`blank_id` ({cfg.blank_id}) must be a class in 0..{cfg.num_classes - 1}")
    if not isinstance(cfg.padding_idx, bool):
        raise ValueError("`padding_idx` must be a bool, as the reference's MultiHeadEmbedding takes it")


def weight_names(cfg: ProbeConfig) -> list:
    """The state-dict keys of a probe of this configuration, torch's names."""
    names = []
    if cfg.pooling is not None:
        names.append("embedding.weight")
    if cfg.pooling == "linear" and cfg.num_codebooks > 1:
        names.append("pooling.mlp.weight")
    if cfg.pooling == "attentional":
        names += ["pooling.attn_mlp.0.weight", "pooling.attn_mlp.0.bias", "pooling.attn_mlp.2.weight"]
    for l in range(cfg.num_layers):
        for sfx in ("", "_reverse"):
            names += [f"encoder.rnn.{p}_l{l}{sfx}" for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    return names + ["head.weight", "head.bias"]


def fold_attn_scores(table: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, w2: torch.Tensor, rows: int) -> torch.Tensor:
    """AttentionalPooling's score ``w2 . relu(W1 e + b1)`` of every row e of the embedding table: it depends on the id alone.  Computed
    in fp64 and rounded once to fp32, as `llama.fold_input` does -> [rows + 2] with `rows` = K C: the codes' scores, then entry K C, the
    padding row's (a zero row's where the table has none), then entry K C + 1, the score of a zero row, which an id out of range reads."""
    t = table.detach().cpu().double()
    w1, b1, w2 = w1.detach().cpu().double(), b1.detach().cpu().double(), w2.detach().cpu().double().reshape(-1)
    score = torch.relu(t @ w1.T + b1) @ w2
    zero = torch.relu(b1) @ w2
    kc = rows
    out = torch.empty(kc + 2, dtype=torch.float64)
    out[:kc] = score[:kc]
    out[kc] = score[kc] if score.numel() > kc else zero
    out[kc + 1] = zero
    return out.to(torch.float32).contiguous()


def relative_to_frames(length: torch.Tensor, N: int) -> torch.Tensor:
    """Relative lengths [B] in 0..1 -> absolute frame counts [B] int64: round(length * N), on the tensor's device.  (speechbrain's own
    helper is not pinned: this is its documented rule.)"""
    return torch.round(length.to(torch.float64) * N).to(torch.int64)


@dataclass
class ProbeOutput:
    """What `TokenProbe.forward` returns; every tensor stays on the device.  CTC head: `frame_pred` [B, N] (-1 beyond a length), `hyp_toks`
    [B, N] (left-packed, -1 filled), `hyp_lens` [B], and `log_probs` [B, N, num_classes] only with `return_stages`.  Utterance head:
    `log_probs` [B, num_classes] and `pred` [B].  `stages`: "pooled" [B, N, E], "layer_out" [layers, B, N, 2 H], "logits"."""
    frame_pred: Optional[torch.Tensor] = None
    hyp_toks: Optional[torch.Tensor] = None
    hyp_lens: Optional[torch.Tensor] = None
    log_probs: Optional[torch.Tensor] = None
    pred: Optional[torch.Tensor] = None
    stages: Optional[dict] = field(default=None)

    def hyps(self) -> list:
        """The decoded sequences as lists (SYNCHRONISES)."""
        lens = self.hyp_lens.cpu().tolist()
        toks = self.hyp_toks.cpu()
        return [toks[i, :n].tolist() for i, n in enumerate(lens)]


def _struct(cfg: ProbeConfig) -> _native.AcProbeConfig:
    check_config(cfg)
    s = _native.AcProbeConfig()
    s.vocab_size, s.num_codebooks, s.embedding_dim, s.hidden_size, s.num_layers = cfg.vocab_size, cfg.num_codebooks, cfg.embedding_dim, cfg.hidden_size, cfg.num_layers
    s.pooling, s.head, s.num_classes, s.blank_id, s.padding_idx = POOLINGS[cfg.pooling], HEADS[cfg.head], cfg.num_classes, cfg.blank_id, int(cfg.padding_idx)
    return s


class TokenProbe(_native.HandleOwner):
    """The recipes' probe (module docstring).  `state_dict` has torch's keys (`weight_names`); `config` is a `ProbeConfig`.  The weights
    are packed once per device, on the first call there."""

    def __init__(self, *, state_dict, config: ProbeConfig = PROBE_RECIPE, precision=None):
        check_config(config)
        if _native.check_precision(precision) == "fp32_exact":
            raise ValueError("a TokenProbe runs in split16 arithmetic only: exact-product mode (\"fp32_exact\") has no row-mode GEMM")
        self.config = cfg = config
        self.precision = precision
        missing = [k for k in weight_names(cfg) if k not in state_dict]
        if missing:
            raise KeyError(f"the state dict lacks {len(missing)} keys of a TokenProbe of this configuration, first: {missing[:3]}")
        w = {k: state_dict[k] for k in weight_names(cfg)}
        H = cfg.hidden_size
        want = {"head.weight": (cfg.num_classes, cfg.head_in), "head.bias": (cfg.num_classes,)}
        if cfg.pooling is not None:
            want["embedding.weight"] = (cfg.table_rows, cfg.embedding_dim)
        for l in range(cfg.num_layers):
            for sfx in ("", "_reverse"):
                want[f"encoder.rnn.weight_ih_l{l}{sfx}"] = (4 * H, cfg.embedding_dim if l == 0 else 2 * H)
                want[f"encoder.rnn.weight_hh_l{l}{sfx}"] = (4 * H, H)
        for k, shape in want.items():
            if tuple(w[k].shape) != shape:
                raise ValueError(f"`{k}` must be {list(shape)}, not {list(w[k].shape)}")
        if cfg.pooling == "linear" and cfg.num_codebooks > 1:
            if w["pooling.mlp.weight"].numel() != cfg.num_codebooks:
                raise ValueError(f"`pooling.mlp.weight` must be [1, {cfg.num_codebooks}]")
            w["pooling.mlp.weight"] = w["pooling.mlp.weight"].reshape(-1)
        if cfg.pooling == "attentional":
            w["pooling.score"] = fold_attn_scores(w["embedding.weight"], w.pop("pooling.attn_mlp.0.weight"), w.pop("pooling.attn_mlp.0.bias"),
                                                  w.pop("pooling.attn_mlp.2.weight"), cfg.vocab_size * cfg.num_codebooks)
        self._weights = w
        self._natives = {}

    def _new_handle(self, device: torch.device) -> _native.Handle:
        return _native.Handle("ac_probe_create", _struct(self.config),
                              "hidden_size one of 32, 64, 128, 256, 512; embedding_dim a multiple of 32; 1..8 layers; 1..32 codebooks", self._weights, device,
                              self.precision)

    def poll(self, device=None) -> None:
        """Surface device-side findings of earlier calls (an id out of range) now: SYNCHRONISES the current stream and raises
        `NativeError` when the handle's sticky words are set; the words are cleared by the report."""
        for nat in self._natives.values():
            if device is not None and nat.device != torch.device(device):
                continue
            with torch.cuda.device(nat.device):
                _native.check(nat.lib.ac_poll_status(nat.h, _native._stream()), nat.h, "ac_poll_status")

    @torch.no_grad()
    def forward(self, toks_or_feats: torch.Tensor, lengths: torch.Tensor = None, return_stages: bool = False, *, _chunk_clips: int = None) -> ProbeOutput:
        """`toks_or_feats`: [B, N, K] integer ids, or [B, N, embedding_dim] fp32 features when the configuration has no pooling.  `lengths`
        is a device int64 [B] of absolute frame counts (None: all N frames); the kernels clamp it into 0..N.  Nothing is read back, and
        the call may be captured into a graph once it ran plain on that device.  An id equal to `vocab_size` with `padding_idx` reads
        the table's extra row; any other id outside [0, vocab_size) reads a zero row and raises the handle's sticky bad-token word
        (`poll`).  `_chunk_clips` (developer argument) forces the clips per pass; the results do not depend on it."""
        cfg = self.config
        x = toks_or_feats
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError("the input must be a [B, N, K] tensor of ids or a [B, N, E] tensor of features with B, N >= 1")
        B, N = int(x.shape[0]), int(x.shape[1])
        if cfg.pooling is None:
            if x.dtype != torch.float32 or x.shape[2] != cfg.embedding_dim:
                raise ValueError(f"without pooling the input must be [B, N, {cfg.embedding_dim}] fp32 features")
        elif x.is_floating_point() or x.dtype == torch.bool or x.shape[2] != cfg.num_codebooks:
            raise ValueError(f"`toks` must be [B, N, {cfg.num_codebooks}] of an integer dtype")
        _host.need_cuda(x.is_cuda, "probe", "input")
        dev = x.device
        if lengths is not None:
            if not torch.is_tensor(lengths) or lengths.dtype != torch.int64 or tuple(lengths.shape) != (B,) or lengths.device != dev:
                raise ValueError(f"`lengths` must be an int64 [{B}] tensor of absolute frame counts on {dev}")
            lengths = lengths.contiguous()
        if _chunk_clips is not None and (isinstance(_chunk_clips, bool) or not isinstance(_chunk_clips, int) or _chunk_clips < 1):
            raise ValueError("`_chunk_clips` must be a positive int")
        nat = self._native_for(x)
        x = (x if cfg.pooling is None else x.to(torch.int64)).contiguous()
        H, NC = cfg.hidden_size, cfg.num_classes
        new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)      # noqa: E731
        out = ProbeOutput()
        if cfg.head == "ctc":
            out.frame_pred, out.hyp_toks, out.hyp_lens = new(B, N, dtype=torch.int64), new(B, N, dtype=torch.int64), new(B, dtype=torch.int64)
            if return_stages:
                out.log_probs = new(B, N, NC)
        else:
            out.log_probs, out.pred = new(B, NC), new(B, dtype=torch.int64)
        if return_stages:
            out.stages = {"layer_out": new(cfg.num_layers, B, N, 2 * H), "logits": new(B, N, NC) if cfg.head == "ctc" else new(B, NC)}
            if cfg.pooling is not None:
                out.stages["pooled"] = new(B, N, cfg.embedding_dim)
        st = out.stages or {}
        o = _native.AcProbeOutputs(*(_native._ptr(t) for t in (out.frame_pred, out.hyp_toks, out.hyp_lens, out.log_probs, out.pred, st.get("pooled"),
                                                               st.get("layer_out"), st.get("logits"))))
        need = int(nat.lib.ac_probe_workspace_bytes(nat.h, B if _chunk_clips is None else min(B, _chunk_clips), N))
        with torch.cuda.device(dev):
            ws = nat.workspace(need + 256)
            rc = nat.lib.ac_probe_forward(nat.h, _native._ptr(x), B, N, _native._ptr(lengths), C.byref(o), _native._ptr(ws), need + 256, _native._stream())
        _native.check(rc, nat.h, "ac_probe_forward")
        return out

    __call__ = forward
