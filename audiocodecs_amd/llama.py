"""The Llama decoder with a KV cache and its token generation loop: the reference's ``LlamaDecoder``
(downstream/models/llama3.py; ``generate`` is called from downstream/train_tts.py:133-150 and downstream/train_slm.py:98-123) as one
handle kind of the HIP library (``ac_lm_create`` / ``ac_lm_forward`` / ``ac_lm_step``).  Inference only, fp32.  There is no CPU fallback.

``LlamaDecoder(state_dict=..., config=...)`` takes the model's own state-dict key layout.  The rotary table is built here, on the CPU,
with the model's own three fp32 torch operations and uploaded as one more weight (at position 8000 the rounding of the fp32 angle is
about 5e-4 rad: a kernel that recomputed the angle would not reproduce it).

``generate`` is the loop of ``_greedy_search``: prefill over ``[prompt | bos_toks]``, then per step a draw from the last row's logits by
``sample_tokens``' rule (``top_p == 0`` is argmax), ``hyp[:, s] = tok``, ``alive &= tok != eos_id``, ``lens[alive] += 1``, and
``embed(tok, curr_pos=s + 1)`` as the next input.  The draw of row ``r`` at step ``s`` is element ``offset + s * B + r`` of the
``"sample"`` stream of ``seed`` (prng.py); ``seed`` is required and no global RNG is read.  The steps run as replays of one captured,
strictly linear graph of ``STEPS_PER_REPLAY`` steps which reads its position from the state; ``alive`` is polled with a non-blocking copy
once per replay, never per token, and steps that run after every row has ended change nothing that is returned.

``score`` is the teacher-forced pass of the recipes' validation and test loops: one causal forward over
``[prompt | toks]`` on the matrix pipe, the log-probability of every target and the arg-max of every row, without logits in memory.

With ``input_dim`` set (the recipes' task files) the checkpoint has ``tok_embeddings.weight`` of that width and the ``input`` Linear behind
it; the two are folded on the host into the one ``[num_codebooks * vocab_size, dim]`` table the library reads (`fold_input`).

Refused (none of the recipes uses them): a finite ``eos_threshold``, ``use_kv_cache=False``, ``batch_parallel=False``, a mask other than
``"causal"``, ``embedding_kwargs``, a prompt whose length is no multiple of ``num_codebooks``, prompt + ``bos_toks`` + ``max_gen_toks``
beyond ``2 * max_seq_len`` (where the reference's rotary table ends), a vocabulary outside the sampler's 2..16384 and more than 64 rows
per state.  The reference's doubling of the cache is not reproduced: a state is allocated once with a capacity, and a row that would
pass it is refused.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, replace
from typing import Optional

import torch

from . import _metric_host as _host
from . import _native
from . import prng
from .sampling import MAX_VOCAB, MIN_VOCAB, STREAM

__all__ = ["LlamaConfig", "LLAMA_TTS", "LLAMA_TINY", "LlamaDecoder", "LlamaState", "LlamaScore", "IGNORE", "stack_generated", "rope_table", "fold_input", "MAX_ROWS",
           "STEPS_PER_REPLAY"]

MAX_ROWS = 64               # rows (batch entries) per state
STEPS_PER_REPLAY = 16       # generated tokens per graph replay = per poll of `alive`
IGNORE = -1                 # a target of `score` that marks an unscored position (any id outside [0, vocab_size) does)


@dataclass(frozen=True)
class LlamaConfig:
    """The arguments of the reference's ``LlamaDecoder`` that the library depends on."""

    vocab_size: int = 1026
    n_layers: int = 12
    dim: int = 512
    ffn_dim: Optional[int] = 2048
    n_heads: int = 4
    n_kv_heads: int = 1
    norm_eps: float = 1e-6
    rope_theta: float = 10000.0
    max_seq_len: int = 8192
    prompt_dim: Optional[int] = None
    num_codebooks: int = 2
    embedding_kwargs: Optional[dict] = None
    input_dim: Optional[int] = None

    @property
    def head_dim(self) -> int:
        return self.dim // self.n_heads

    @property
    def ffn(self) -> int:
        return 4 * self.dim if self.ffn_dim is None else self.ffn_dim


# hparams/_legacy/tts/LibriSpeech/encodec.yaml:76-99,134-144: vocabulary 1024 + 2, 2 codebooks; `prompt_dim` is the caller's (the speaker
# embedding's width): LlamaDecoder(config=dataclasses.replace(LLAMA_TTS, prompt_dim=512), ...)
LLAMA_TTS = LlamaConfig()
LLAMA_TINY = LlamaConfig(vocab_size=130, n_layers=2, dim=64, ffn_dim=128, n_heads=4, n_kv_heads=1, max_seq_len=512, prompt_dim=24, num_codebooks=2)


def rope_table(cfg: LlamaConfig):
    """(cos, sin) [2 * max_seq_len, head_dim / 2] fp32 of the reference's ``freqs_cis`` (llama3.py:618-632), with its own operations."""
    hd = cfg.head_dim
    freqs = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2)[: hd // 2].float() / hd))
    t = torch.arange(2 * cfg.max_seq_len, dtype=torch.float32)
    cis = torch.polar(torch.ones(len(t), len(freqs)), torch.outer(t, freqs))
    return cis.real.contiguous(), cis.imag.contiguous()


def _check_config(cfg: LlamaConfig) -> None:
    if not isinstance(cfg, LlamaConfig):
        raise ValueError("`config` must be a LlamaConfig")
    if cfg.embedding_kwargs:
        raise NotImplementedError("`embedding_kwargs` (a padding row, max_norm, ...) are not compiled")
    if isinstance(cfg.vocab_size, bool) or not isinstance(cfg.vocab_size, int) or not MIN_VOCAB <= cfg.vocab_size <= MAX_VOCAB:
        raise ValueError(f"`vocab_size` ({cfg.vocab_size!r}) must be in the sampler's range {MIN_VOCAB}..{MAX_VOCAB}")


def _struct(cfg: LlamaConfig) -> _native.AcLmConfig:
    _check_config(cfg)
    c = _native.AcLmConfig()
    c.vocab_size, c.n_layers, c.dim, c.ffn_dim, c.n_heads, c.n_kv_heads = cfg.vocab_size, cfg.n_layers, cfg.dim, cfg.ffn, cfg.n_heads, cfg.n_kv_heads
    c.max_seq_len, c.prompt_dim, c.num_codebooks = cfg.max_seq_len, cfg.prompt_dim or 0, cfg.num_codebooks
    c.norm_eps, c.rope_theta = float(cfg.norm_eps), float(cfg.rope_theta)
    return c


def weight_names(cfg: LlamaConfig):
    """The state-dict keys a `LlamaDecoder` of `cfg` needs."""
    names = ["tok_embeddings.weight", "norm.weight"]
    names += [f"output.{k}.weight" for k in range(cfg.num_codebooks)] if cfg.num_codebooks > 1 else ["output.weight"]
    if cfg.prompt_dim:
        names.append("prompt.weight")
    if cfg.input_dim is not None:
        names.append("input.weight")
    for l in range(cfg.n_layers):
        names += [f"layers.{l}.attention.{w}.weight" for w in ("wq", "wk", "wv", "wo")]
        names += [f"layers.{l}.feed_forward.{w}.weight" for w in ("w1", "w2", "w3")]
        names += [f"layers.{l}.attention_norm.weight", f"layers.{l}.ffn_norm.weight"]
    return names


def fold_input(table: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``input(tok_embeddings(tok))`` as one table: `table` [rows, input_dim] times `weight` [dim, input_dim] transposed, the product in
    fp64 and rounded once to fp32 -- every row of the result is the correctly rounded embedding of its id."""
    if table.dim() != 2 or weight.dim() != 2 or table.shape[1] != weight.shape[1]:
        raise ValueError(f"`tok_embeddings.weight` {tuple(table.shape)} and `input.weight` {tuple(weight.shape)} do not share the width input_dim")
    return (table.detach().cpu().double() @ weight.detach().cpu().double().T).to(torch.float32).contiguous()


@dataclass
class LlamaScore:
    """What `LlamaDecoder.score` returns; every tensor stays on the device.  `stages` is None unless they were asked for."""

    logp: torch.Tensor          # [B, T] fp32: log_softmax(logits)[target], 0 where unscored
    pred: torch.Tensor          # [B, T] int64: the arg-max of every row's logits, the lowest index on a tie
    sum_logp: torch.Tensor      # [B] fp64: logp summed over the row's scored positions, in a fixed order
    count: torch.Tensor         # [B] int64: scored positions
    errors: torch.Tensor        # [B] int64: scored positions with pred != target
    stages: Optional[dict] = None

    @property
    def nll(self) -> torch.Tensor:
        """Mean negative log-likelihood over all scored positions (the recipes' loss)."""
        return -self.sum_logp.sum() / self.count.sum()

    @property
    def ter(self) -> torch.Tensor:
        """Token error rate of the arg-max over all scored positions."""
        return self.errors.sum().double() / self.count.sum()

    @property
    def mean_logp(self) -> torch.Tensor:
        """[B]: the length-normalised log-probability of every row."""
        return self.sum_logp / self.count


def stack_generated(hyp_toks, num_codebooks: int, vocab_size: int) -> torch.Tensor:
    """The recipes' reshape of `generate`'s result (downstream/train_tts.py:147-153): the rows, of one length N K as `eos_id=-1` returns
    them, stacked to [B, N, K], with the ids at and above `vocab_size` (the codec's: the special ids lie there) set to `vocab_size - 1`."""
    out = torch.stack(list(hyp_toks))
    out = out.reshape(len(out), -1, num_codebooks)
    return out.clamp(max=vocab_size - 1)


class LlamaState:
    """The cache and the counters of one sequence batch on the device: opaque, with `.pos` (rows in the cache), `.B` and `.capacity`."""

    def __init__(self, nat, B: int, capacity: int, max_steps: int, offset: int = 0, zero: bool = False):
        self.nat, self.B, self.capacity, self.max_steps, self.pos = nat, int(B), int(capacity), int(max_steps), 0
        lay = _native.AcLmLayout()
        _native.check(nat.lib.ac_lm_state_layout(nat.h, self.B, self.capacity, self.max_steps, C.byref(lay)), nat.h, "ac_lm_state_layout")
        self.layout = lay
        self.buf = (torch.zeros if zero else torch.empty)(int(lay.total), dtype=torch.uint8, device=nat.device)
        self.ws = None
        with torch.cuda.device(nat.device):
            rc = nat.lib.ac_lm_reset(nat.h, _native._ptr(self.buf), self.buf.numel(), self.B, self.capacity, self.max_steps, int(offset), _native._stream())
        _native.check(rc, nat.h, "ac_lm_reset")

    def _view(self, off: int, count: int, dtype) -> torch.Tensor:
        size = torch.empty(0, dtype=dtype).element_size()
        return self.buf[off:off + count * size].view(dtype)

    def header(self) -> torch.Tensor:
        """[64] int32: position, -, step, -, overflow flag, ... (include/audiocodecs_amd.h)."""
        return self._view(self.layout.hdr, 64, torch.int32)

    def check(self):
        """The header on the host (SYNCHRONISES); raises when a step or a forward found the state full or not the caller's."""
        head = self.header().cpu().tolist()
        if head[4] != 0:
            raise _native.NativeError("the state's flag word is set: a step would have passed its capacity of "
                                      f"{self.capacity} positions (or a call did not match the state); nothing was written for it")
        return head

    def alive(self) -> torch.Tensor:
        return self._view(self.layout.alive, self.B, torch.int32)

    def lens(self) -> torch.Tensor:
        return self._view(self.layout.lens, self.B, torch.int32)

    def logits(self, vocab: int) -> torch.Tensor:
        return self._view(self.layout.logits, self.B * vocab, torch.float32).view(self.B, vocab)

    def hyp(self) -> torch.Tensor:
        return self._view(self.layout.hyp, self.B * self.max_steps, torch.int64).view(self.B, self.max_steps)

    def kv(self, layer: int, n_kv_heads: int, head_dim: int):
        """(K, V) of `layer` as views [B, capacity, n_kv_heads, head_dim]; rows at and beyond `.pos` are not defined."""
        n = self.B * self.capacity * n_kv_heads * head_dim
        at = self.layout.kv + 2 * layer * self.layout.plane_bytes
        shape = (self.B, self.capacity, n_kv_heads, head_dim)
        return self._view(at, n, torch.float32).view(shape), self._view(at + self.layout.plane_bytes, n, torch.float32).view(shape)

    def workspace(self, T: int) -> torch.Tensor:
        need = int(self.nat.lib.ac_lm_workspace_bytes(self.nat.h, self.B, int(T), self.capacity))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=self.nat.device)
        return self.ws


class LlamaDecoder(_native.HandleOwner):
    """The reference's ``LlamaDecoder`` on the HIP library: ``embed``, ``forward`` and ``generate`` (the module docstring states what is
    refused).  `state_dict` has the model's own keys; `config` is a `LlamaConfig`."""

    def __init__(self, *, state_dict, config: LlamaConfig = LLAMA_TTS):
        _struct(config)
        self.config = config
        missing = [k for k in weight_names(config) if k not in state_dict]
        if missing:
            raise KeyError(f"the state dict lacks {len(missing)} keys of a LlamaDecoder of this configuration, first: {missing[:3]}")
        self._weights = {k: state_dict[k] for k in weight_names(config)}
        if config.input_dim is not None:      # the library knows one table of width dim: E @ W^T
            if tuple(self._weights["tok_embeddings.weight"].shape) != (config.num_codebooks * config.vocab_size, config.input_dim):
                raise ValueError(f"`tok_embeddings.weight` must be [{config.num_codebooks * config.vocab_size}, {config.input_dim}] with input_dim set")
            self._weights["tok_embeddings.weight"] = fold_input(self._weights["tok_embeddings.weight"], self._weights.pop("input.weight"))
        self._scoring = set()
        self._weights["lm.rope_cos"], self._weights["lm.rope_sin"] = rope_table(config)
        self._natives = {}
        self._warm = set()

    def _new_handle(self, device: torch.device) -> _native.Handle:
        return _native.Handle("ac_lm_create", _struct(self.config),
                              "dim % n_heads, n_heads % n_kv_heads with 1, 2, 4 or 8 query heads per key/value head, an even head dim <= 256, "
                              "dim / ffn_dim / prompt_dim multiples of 4, vocab_size in 2..16384", self._weights, device)

    # ---- embed ---------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def embed(self, toks: torch.Tensor, prompt_embs: torch.Tensor = None, curr_pos: int = 0) -> torch.Tensor:
        """`toks` [B, T] integer ids, `prompt_embs` [B, P, prompt_dim or dim] or None -> [B, P + T, dim] fp32: token j reads row
        ``tok + ((curr_pos + j) % num_codebooks) * vocab_size`` of the table; prompt rows of width `prompt_dim` go through the
        ``prompt`` Linear and are prepended."""
        cfg = self.config
        if not torch.is_tensor(toks) or toks.dim() != 2 or toks.is_floating_point() or toks.dtype == torch.bool:
            raise ValueError("`toks` must be a [B, T] tensor of an integer dtype")
        if isinstance(curr_pos, bool) or not isinstance(curr_pos, int) or curr_pos < 0:
            raise ValueError(f"`curr_pos` ({curr_pos!r}) must be a non-negative int")
        B, T = (int(n) for n in toks.shape)
        P, width = 0, 0
        if prompt_embs is not None:
            if not torch.is_tensor(prompt_embs) or prompt_embs.dim() != 3 or prompt_embs.shape[0] != B or prompt_embs.dtype != torch.float32:
                raise ValueError(f"`prompt_embs` must be a [{B}, P, width] fp32 tensor")
            P, width = int(prompt_embs.shape[1]), int(prompt_embs.shape[2])
            if width != (cfg.prompt_dim or -1) and width != cfg.dim:
                raise ValueError(f"`prompt_embs` has width {width}: neither prompt_dim ({cfg.prompt_dim}) nor dim ({cfg.dim})")
        if B < 1 or T + P < 1:
            raise ValueError("nothing to embed")
        _host.need_cuda(toks.is_cuda and (prompt_embs is None or prompt_embs.is_cuda), "llama", "tokens and the prompt")
        nat = self._native_for(toks)
        out = torch.empty(B, P + T, cfg.dim, dtype=torch.float32, device=toks.device)
        t64 = toks.to(torch.int64).contiguous()
        pe = prompt_embs.contiguous() if P else None
        with torch.cuda.device(toks.device):
            rc = nat.lib.ac_lm_embed(nat.h, _native._ptr(t64) if T else None, B, T, curr_pos, _native._ptr(pe), P, width, _native._ptr(out), _native._stream())
        _native.check(rc, nat.h, "ac_lm_embed")
        return out

    # ---- score ---------------------------------------------------------------------------------------------------------------------
    def _check_score(self, toks, targets, prompt_embs, lengths):
        """The refusals of `score` that need no device -> (B, T, P)."""
        cfg = self.config
        if not torch.is_tensor(toks) or toks.dim() != 2 or toks.is_floating_point() or toks.dtype == torch.bool or toks.shape[0] < 1 or toks.shape[1] < 1:
            raise ValueError("`toks` must be a [B, T] tensor of an integer dtype with B, T >= 1")
        B, T = (int(n) for n in toks.shape)
        if not torch.is_tensor(targets) or targets.dtype != torch.int64 or tuple(targets.shape) != (B, T):
            raise ValueError(f"`targets` must be a [{B}, {T}] int64 tensor")
        P = 0
        if prompt_embs is not None:
            if not torch.is_tensor(prompt_embs) or prompt_embs.dim() != 3 or prompt_embs.shape[0] != B or prompt_embs.dtype != torch.float32:
                raise ValueError(f"`prompt_embs` must be a [{B}, P, width] fp32 tensor")
            P = int(prompt_embs.shape[1])
            if P % cfg.num_codebooks:
                raise ValueError(f"a prompt of {P} rows is no multiple of num_codebooks ({cfg.num_codebooks})")
        if P + T > 2 * cfg.max_seq_len:
            raise ValueError(f"prompt + toks = {P + T} positions pass 2 * max_seq_len = {2 * cfg.max_seq_len}, where the rotary table ends")
        if lengths is not None:
            if torch.is_tensor(lengths):
                if lengths.is_floating_point() or lengths.dtype == torch.bool or tuple(lengths.shape) != (B,):
                    raise ValueError(f"`lengths` must be [{B}] integers")
                host = None if lengths.is_cuda else lengths.tolist()
            else:
                host = list(lengths)
                if len(host) != B or any(isinstance(n, bool) or not isinstance(n, int) for n in host):
                    raise ValueError(f"`lengths` must be [{B}] integers")
            if host is not None and any(not 0 <= n <= T for n in host):
                raise ValueError(f"`lengths` must lie in 0..{T}")
        return B, T, P

    @torch.no_grad()
    def score(self, toks: torch.Tensor, targets: torch.Tensor, *, prompt_embs: torch.Tensor = None, lengths=None, return_stages: bool = False,
              _chunk_clips: int = None) -> LlamaScore:
        """Teacher-forced scoring: one causal forward over ``embed(toks, prompt_embs, 0)``; position t of row b is scored against
        ``targets[b, t]`` (int64) from the logits of row ``P + t``.  A target outside ``[0, vocab_size)`` (`IGNORE`) and positions
        ``t >= lengths[b]`` are unscored.  `lengths` is [B] integers: given on the host they are checked against 0..T; a device tensor is
        not read back, the kernels clamp it into 0..T.  Nothing is read back and the call may be captured into a graph once it ran plain
        on that device.  `return_stages` adds, per layer, the rotated "q" and "k", "attn" and "layer_out" over all P + T rows, then
        "final_norm" and the "logits" [B, T, vocab_size] of the token rows (for tests).  `_chunk_clips` (developer argument) forces the
        clips per pass; the results do not depend on it."""
        cfg = self.config
        B, T, P = self._check_score(toks, targets, prompt_embs, lengths)
        _host.need_cuda(toks.is_cuda and targets.is_cuda, "llama", "tokens and targets")
        if targets.device != toks.device:
            raise ValueError(f"`targets` ({targets.device}) and `toks` ({toks.device}) must be on one device")
        embs = self.embed(toks, prompt_embs if P else None, 0)
        dev, Ttot = embs.device, P + T
        nat = self._native_for(embs)
        if dev.index not in self._scoring:
            with torch.cuda.device(dev):
                _native.check(nat.lib.ac_lm_prepare_score(nat.h), nat.h, "ac_lm_prepare_score")
            self._scoring.add(dev.index)
        tg = targets.contiguous()
        ln = None
        if lengths is not None:
            ln = (lengths if torch.is_tensor(lengths) else torch.tensor(lengths, dtype=torch.int64)).to(device=dev, dtype=torch.int64).contiguous()
        out = LlamaScore(torch.empty(B, T, dtype=torch.float32, device=dev), torch.empty(B, T, dtype=torch.int64, device=dev),
                         torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev))
        st = None
        if return_stages:
            nq, nkvd, L = cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim, cfg.n_layers
            new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)      # noqa: E731
            out.stages = {"q": new(L, B, Ttot, nq), "k": new(L, B, Ttot, nkvd), "attn": new(L, B, Ttot, nq), "layer_out": new(L, B, Ttot, cfg.dim),
                          "final_norm": new(B, Ttot, cfg.dim), "logits": new(B, T, cfg.vocab_size)}
            st = _native.AcLmScoreStages(*(out.stages[k].data_ptr() for k in ("q", "k", "attn", "layer_out", "final_norm", "logits")))
        if _chunk_clips is not None and (isinstance(_chunk_clips, bool) or not isinstance(_chunk_clips, int) or _chunk_clips < 1):
            raise ValueError("`_chunk_clips` must be a positive int")
        need = int(nat.lib.ac_lm_score_workspace_bytes(nat.h, B if _chunk_clips is None else min(B, _chunk_clips), Ttot))
        with torch.cuda.device(dev):
            ws = nat.workspace(need + 256)
            rc = nat.lib.ac_lm_score(nat.h, _native._ptr(embs), B, P, T, _native._ptr(tg), _native._ptr(ln), _native._ptr(out.logp), _native._ptr(out.pred),
                                     _native._ptr(out.sum_logp), _native._ptr(out.count), _native._ptr(out.errors), C.byref(st) if st is not None else None,
                                     _native._ptr(ws), need + 256, _native._stream())
        _native.check(rc, nat.h, "ac_lm_score")
        return out

    # ---- forward -------------------------------------------------------------------------------------------------------------------
    def new_state(self, B: int, capacity: int, device=None, max_steps: int = 0, offset: int = 0) -> LlamaState:
        """A fresh state of `B` rows whose cache holds `capacity` positions (allocated once; it does not grow)."""
        if isinstance(B, bool) or not isinstance(B, int) or not 1 <= B <= MAX_ROWS:
            raise ValueError(f"a state holds 1..{MAX_ROWS} rows, not {B!r}")
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= 2 * self.config.max_seq_len:
            raise ValueError(f"`capacity` ({capacity!r}) must be in 1..{2 * self.config.max_seq_len} = 2 * max_seq_len, where the rotary table ends")
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return LlamaState(self._native_for(torch.empty(0, device=dev)), B, capacity, max_steps, offset)

    @torch.no_grad()
    def forward(self, embs: torch.Tensor, mask="causal", state: LlamaState = None, return_stages: bool = False, capacity: int = None):
        """`embs` [B, T, dim] fp32 -> (logits [B, T, vocab_size], state): the rows are appended at `state.pos` (a fresh state without one:
        of `capacity` positions, by default 2 T as the reference's first allocation, capped at 2 * max_seq_len) and attend causally to
        everything before them.  The row at absolute position p uses output head ``p % num_codebooks``.  With `return_stages` the
        result is (logits, state, stages): per layer the rotated queries "q" and the attention output "attn" [L, B, T, n_heads *
        head_dim], the layer output "layer_out" [L, B, T, dim], and "final_norm" [B, T, dim]."""
        cfg = self.config
        if mask != "causal":
            raise NotImplementedError("only mask=\"causal\" is compiled")
        if not torch.is_tensor(embs) or embs.dim() != 3 or embs.dtype != torch.float32 or embs.shape[2] != cfg.dim or embs.shape[1] < 1:
            raise ValueError(f"`embs` must be a [B, T, {cfg.dim}] fp32 tensor")
        B, T = int(embs.shape[0]), int(embs.shape[1])
        _host.need_cuda(embs.is_cuda, "llama", "embeddings")
        if state is None:
            state = self.new_state(B, min(2 * T, 2 * cfg.max_seq_len) if capacity is None else capacity, embs.device)
        if not isinstance(state, LlamaState) or state.B != B or state.buf.device != embs.device:
            raise ValueError(f"`state` must be a LlamaState of {B} rows on {embs.device}")
        if state.pos + T > state.capacity:
            raise ValueError(f"rows {state.pos}..{state.pos + T - 1} pass the state's capacity of {state.capacity} positions")
        nat = state.nat
        dev = embs.device
        logits = torch.empty(B, T, cfg.vocab_size, dtype=torch.float32, device=dev)
        stages, st = None, None
        if return_stages:
            nq = cfg.n_heads * cfg.head_dim
            stages = {"q": torch.empty(cfg.n_layers, B, T, nq, dtype=torch.float32, device=dev), "attn": torch.empty(cfg.n_layers, B, T, nq, dtype=torch.float32, device=dev),
                      "layer_out": torch.empty(cfg.n_layers, B, T, cfg.dim, dtype=torch.float32, device=dev), "final_norm": torch.empty(B, T, cfg.dim, dtype=torch.float32, device=dev)}
            st = _native.AcLmStages(*(stages[k].data_ptr() for k in ("q", "attn", "layer_out", "final_norm")))
        x = embs.contiguous()
        with torch.cuda.device(dev):
            ws = state.workspace(T)
            rc = nat.lib.ac_lm_forward(nat.h, _native._ptr(state.buf), state.buf.numel(), B, state.capacity, state.max_steps, state.pos, _native._ptr(x), T,
                                       _native._ptr(logits), C.byref(st) if st is not None else None, _native._ptr(ws), ws.numel(), _native._stream())
        _native.check(rc, nat.h, "ac_lm_forward")
        state.pos += T
        return (logits, state, stages) if return_stages else (logits, state)

    __call__ = forward

    # ---- generate ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, bos_toks: torch.Tensor, eos_id: int, prompt_embs: torch.Tensor = None, max_gen_toks: int = 100, eos_threshold: float = float("inf"),
                 top_p: float = 0.9, temp: float = 1.0, use_kv_cache: bool = True, batch_parallel: bool = True, *, seed, offset: int = 0,
                 return_logits: bool = False, use_graph: bool = True):
        """The reference's ``generate`` -> a list of B int64 tensors ``hyp[i, :lens[i]]`` (the EOS token itself is not part of a row);
        with `return_logits` also the [steps, B, vocab_size] fp32 logits every token was drawn from (steps: those that ran before the
        last row ended).  `use_graph=False` issues the same launches without capturing them (bit-identical; for tests)."""
        cfg = self.config
        if eos_threshold < float("inf"):
            raise NotImplementedError("a finite `eos_threshold` is not compiled")
        if not use_kv_cache or not batch_parallel:
            raise NotImplementedError("`use_kv_cache=False` and `batch_parallel=False` are not compiled")
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError("`seed` must be an int: there is no global RNG")
        if isinstance(offset, bool) or not isinstance(offset, int) or not 0 <= offset < 1 << 62:
            raise ValueError(f"`offset` ({offset!r}) must be an int in [0, 2^62)")
        if isinstance(max_gen_toks, bool) or not isinstance(max_gen_toks, int) or max_gen_toks < 1:
            raise ValueError(f"`max_gen_toks` ({max_gen_toks!r}) must be a positive int")
        if isinstance(eos_id, bool) or not isinstance(eos_id, int):
            raise ValueError("`eos_id` must be an int")
        top_p, temp = float(top_p), float(temp)
        if not 0.0 <= top_p <= 1.0:
            raise ValueError(f"`top_p` ({top_p}) must be in [0, 1]")
        if not 0.0 < temp < float("inf"):
            raise ValueError(f"`temp` ({temp}) must be positive and finite")
        if not torch.is_tensor(bos_toks) or bos_toks.dim() != 2 or bos_toks.shape[1] < 1:
            raise ValueError("`bos_toks` must be a [B, T] tensor of ids")
        B = int(bos_toks.shape[0])
        if not 1 <= B <= MAX_ROWS:
            raise ValueError(f"a state holds 1..{MAX_ROWS} rows, not {B}")
        P = 0
        if prompt_embs is not None:
            P = int(prompt_embs.shape[1]) if torch.is_tensor(prompt_embs) and prompt_embs.dim() == 3 else -1
            if P < 0 or (cfg.num_codebooks > 1 and P % cfg.num_codebooks):
                raise ValueError(f"`prompt_embs` must be [B, P, width] with P a multiple of num_codebooks ({cfg.num_codebooks})")
        T0 = P + int(bos_toks.shape[1])
        if T0 + max_gen_toks > 2 * cfg.max_seq_len:
            raise ValueError(f"prompt + bos_toks + max_gen_toks = {T0 + max_gen_toks} positions pass 2 * max_seq_len = {2 * cfg.max_seq_len}, where the rotary table ends")
        embs = self.embed(bos_toks, prompt_embs if P else None)
        dev = embs.device
        state = self.new_state(B, T0 + max_gen_toks, dev, max_steps=max_gen_toks, offset=offset)
        nat = state.nat
        log = torch.empty(max_gen_toks, B, cfg.vocab_size, dtype=torch.float32, device=dev) if return_logits else None
        self.forward(embs, state=state)
        key = int(prng.key_for(seed, STREAM))
        state.workspace(max(T0, 1))       # (the steps use the buffer the prefill left: no allocation between replays)

        def steps(n):
            for _ in range(n):
                rc = nat.lib.ac_lm_step(nat.h, _native._ptr(state.buf), state.buf.numel(), B, state.capacity, state.max_steps, eos_id, temp, top_p, key,
                                        _native._ptr(log), _native._ptr(state.ws), state.ws.numel(), _native._stream())
                _native.check(rc, nat.h, "ac_lm_step")

        if use_graph and (dev.index, B) not in self._warm:
            # every kernel of a step runs once outside a capture first, on a throwaway state of the same row count (the row count picks
            # the kernels' instances)
            tmp = LlamaState(nat, B, 2, 2, zero=True)
            with torch.cuda.device(dev):
                tmp.workspace(1)
                rc = nat.lib.ac_lm_step(nat.h, _native._ptr(tmp.buf), tmp.buf.numel(), B, 2, 2, eos_id, temp, top_p, key, None, _native._ptr(tmp.ws), tmp.ws.numel(),
                                        _native._stream())
            _native.check(rc, nat.h, "ac_lm_step")
            torch.cuda.current_stream().synchronize()
            self._warm.add((dev.index, B))
        hdr, alive = state.header(), state.alive()
        polled = torch.empty(2, dtype=torch.int32).pin_memory()
        done_event, pending = torch.cuda.Event(), False
        with torch.cuda.device(dev):
            replays = -(-max_gen_toks // STEPS_PER_REPLAY)
            graph = None
            if use_graph and replays > 1:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=side):
                    steps(STEPS_PER_REPLAY)
                torch.cuda.current_stream().wait_stream(side)
                # (the capture ran nothing: the first replay is the first step)
            for _ in range(replays):
                if pending and done_event.query():      # the poll issued behind the replay before: never waits
                    if polled[0].item() == 0 or polled[1].item() != 0:
                        break
                    pending = False
                if graph is not None:
                    graph.replay()
                else:
                    steps(STEPS_PER_REPLAY)
                if not pending:
                    polled[0:1].copy_(alive.sum(dtype=torch.int32).view(1), non_blocking=True)
                    polled[1:2].copy_(hdr[4:5], non_blocking=True)
                    done_event.record()
                    pending = True
            torch.cuda.current_stream().synchronize()
        head = state.check()
        n_steps = int(head[2])
        lens = state.lens().cpu().tolist()
        hyp = state.hyp()
        out = [hyp[i, :lens[i]].clone() for i in range(B)]
        state.pos = int(head[0])
        return (out, log[:n_steps]) if return_logits else out
