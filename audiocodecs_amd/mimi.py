"""Mimi on MI355X -- host-side mirror of the reference wrapper `audiocodecs.Mimi`
(/root/reference/audiocodecs/mimi.py:25-156): same constructor arguments (`sample_rate`, `mode`,
`num_codebooks`, `latent`), attributes (`num_codebooks`, `vocab_size`, `latent`), method names, tensor
layouts and error behaviour.  The third-party `transformers.MimiModel` the reference calls
(mimi.py:45,105,115-119,139,146,153) is replaced by the gfx950 kernels behind the C ABI
(include/audiocodecs_amd.h, ac_mimi_create).  PyTorch is used for device memory and streams only.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _native
from .codec import Codec
from .config import MIMI_24KHZ, MimiConfig
from .encodec import _ptr, _stream
from .resample import ResampleStream
from .sessions import plan_push

__all__ = ["Mimi", "MimiEncodeStream", "MimiDecodeStream", "MimiEncodeSessions", "MimiDecodeSessions"]


class _NativeMimi:
    """One Mimi ac_handle: weights on one GPU + a grow-only workspace tensor."""

    def __init__(self, cfg: MimiConfig, sd: Dict[str, torch.Tensor], device: torch.device, precision=None):
        self.lib = _native.lib()
        c = _native.AcMimiConfig()
        c.struct_size = C.sizeof(_native.AcMimiConfig)
        for f in ("sampling_rate", "num_filters", "hidden_size", "kernel_size", "last_kernel_size", "residual_kernel_size",
                  "compress", "codebook_size", "codebook_dim", "num_quantizers", "num_semantic_quantizers", "num_hidden_layers",
                  "num_attention_heads", "head_dim", "intermediate_size", "sliding_window", "resample_stride"):
            setattr(c, f, getattr(cfg, f))
        c.num_ratios = len(cfg.upsampling_ratios)
        for i, r in enumerate(cfg.upsampling_ratios):
            c.upsampling_ratios[i] = r
        c.rope_theta = cfg.rope_theta
        c.norm_eps = cfg.norm_eps
        c.device = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", c.device)
        self.h = C.c_void_p()
        rc = self.lib.ac_mimi_create(C.byref(c), C.byref(self.h))
        if rc < 0:
            raise _native.NativeError(f"ac_mimi_create failed with code {rc} (is a gfx950 GPU visible?)")
        _native.set_precision(self.lib, self.h, precision)
        for name, t in sd.items():
            if not t.is_floating_point() or name.endswith(".initialized"):
                continue
            t = t.detach().to(torch.float32).cpu().contiguous()
            _native.check(
                self.lib.ac_load_weights(self.h, name.encode(), C.c_void_p(t.data_ptr()), t.numel() * 4),
                self.h, f"ac_load_weights({name})",
            )
        with torch.cuda.device(self.device):
            _native.check(self.lib.ac_finalize(self.h), self.h, "ac_finalize")
        self.ws: Optional[torch.Tensor] = None
        _native.track(self)

    def workspace(self, nbytes: int) -> torch.Tensor:
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return self.ws

    def __del__(self):
        try:
            import sys

            if sys.is_finalizing():   # interpreter shutdown: the HIP runtime may already be gone, the OS reclaims the rest
                return
            if getattr(self, "h", None):
                self.lib.ac_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Mimi(Codec):
    _accepts_none_length = True

    def __init__(
        self,
        sample_rate,
        mode="reconstruct",
        num_codebooks=8,
        latent=True,
        *,
        state_dict: Optional[Dict[str, torch.Tensor]] = None,
        config: MimiConfig = MIMI_24KHZ,
        precision: Optional[str] = None,
        strict: bool = False,
        graph: bool = False,
    ):
        """`state_dict`: an HF-format MimiModel state dict (`safetensors.torch.load_file` of kyutai/mimi's
        model.safetensors, or `checkpoint.synthetic_mimi_state_dict(cfg, seed)`); fetched through
        huggingface_hub like the reference when omitted (needs network or a warm cache)."""
        super().__init__(sample_rate, config.sampling_rate, mode)  # mimi.py:38
        self.strict = bool(strict)   # codec.py: poll the handle after every call
        self.graph = bool(graph)     # codec.py: replay one hipGraph per (call, shape)
        self.num_codebooks = num_codebooks
        self.vocab_size = config.codebook_size  # 2048 (mimi.py:40)
        self.latent = latent
        self.config = config
        self.precision = _native.check_precision(precision)   # see Encodec: None / "fp32" (parity arithmetic), "fp32_exact"
        if state_dict is None:
            state_dict = self._fetch_pretrained()
        self._sd = {k: v for k, v in state_dict.items()}
        self._natives: Dict[int, _NativeMimi] = {}

    @staticmethod
    def _fetch_pretrained():
        try:
            from huggingface_hub import hf_hub_download
            from safetensors.torch import load_file
        except ImportError:
            raise ImportError("`pip install huggingface_hub safetensors` to fetch pretrained Mimi weights")
        return load_file(hf_hub_download("kyutai/mimi", "model.safetensors"))

    # ------------------------------------------------------------------------------------------
    def _native_for(self, t: torch.Tensor) -> _NativeMimi:
        if not t.is_cuda:
            raise _native.NativeError(
                "audiocodecs_amd runs on MI355X only: move the input to a cuda device "
                "(there is deliberately no CPU fallback)"
            )
        idx = t.device.index
        if idx not in self._natives:
            self._natives[idx] = _NativeMimi(self.config, self._sd, t.device, self.precision)
        return self._natives[idx]

    def _any_native(self) -> _NativeMimi:
        dev = next(iter(self._natives.values())).device if self._natives else torch.device("cuda", torch.cuda.current_device())
        return self._native_for(torch.empty(0, device=dev))

    def _check_num_codebooks(self):
        """[HF] mimi :1106-1114 (SplitResidualVectorQuantizer.encode) / :1330-1333 (MimiModel.encode)."""
        K, nq, nsem = self.num_codebooks, self.config.num_quantizers, self.config.num_semantic_quantizers
        if K > nq:
            raise ValueError(
                f"The number of quantizers (i.e codebooks) asked should be lower than the total number of quantizers {nq}, but is currently {K}."
            )
        if K < nsem:
            raise ValueError(
                f"The number of quantizers (i.e codebooks) asked should be higher than the number of semantic quantizers {nsem}, but is currently {K}."
            )

    # override
    @torch.no_grad()
    def embs(self):
        nat = self._any_native()
        K = self.num_codebooks
        width = self.config.codebook_dim if self.latent else self.config.hidden_size
        out = torch.empty(K, self.vocab_size, width, device=nat.device)
        with torch.cuda.device(nat.device):
            fn = nat.lib.ac_embs if self.latent else nat.lib.ac_embs_projected
            _native.check(fn(nat.h, K, _ptr(out), _stream()), nat.h, "ac_embs")
        return out  # [K, C, D] (latent) or [K, C, hidden]

    # override
    def _sig_to_toks(self, sig, length):
        # sig: [B, T].  The padding mask the reference builds (mimi.py:95-104) is not applied to the
        # samples by the model ([HF] mimi :1245-1247): `length` does not change the result.
        self._check_num_codebooks()
        B, T = sig.shape
        K = self.num_codebooks
        N = self.config.num_frames(T)
        if B == 0:   # an empty shard (sharding.shard_bounds): nothing to run, the library is not called
            return torch.empty(0, N, K, dtype=torch.int64, device=sig.device)
        nat = self._native_for(sig)
        sig = sig.to(torch.float32).contiguous()
        toks = torch.empty(B, N, K, dtype=torch.int64, device=sig.device)
        with torch.cuda.device(nat.device):
            ws = nat.workspace(nat.lib.ac_encode_workspace_bytes(nat.h, B, T))
            _native.check(
                nat.lib.ac_encode(nat.h, _ptr(sig), None, B, T, K, _ptr(toks), _ptr(ws), ws.numel(), _stream()),
                nat.h, "ac_encode",
            )
        return toks  # [B, N, K]

    # override
    def _sig_to_feats(self, sig, length):
        # sig: [B, T] -> [B, N, hidden]: encoder -> encoder_transformer -> downsample (mimi.py:112-121)
        B, T = sig.shape
        N = self.config.num_frames(T)
        if B == 0:
            return torch.empty(0, N, self.config.hidden_size, dtype=torch.float32, device=sig.device)
        nat = self._native_for(sig)
        sig = sig.to(torch.float32).contiguous()
        feats = torch.empty(B, N, self.config.hidden_size, dtype=torch.float32, device=sig.device)
        with torch.cuda.device(nat.device):
            ws = nat.workspace(nat.lib.ac_encode_workspace_bytes(nat.h, B, T))
            _native.check(
                nat.lib.ac_encode_feats(nat.h, _ptr(sig), None, B, T, _ptr(feats), _ptr(ws), ws.numel(), _stream()),
                nat.h, "ac_encode_feats",
            )
        return feats

    # override
    def _sig_to_qfeats(self, sig, length):
        return self._toks_to_qfeats(self._sig_to_toks(sig, length), length)

    # override
    def _toks_to_sig(self, toks, length):
        # toks: [B, N, K] -> [B, N*hop] (not trimmed: mimi.py:146-148 passes no padding mask)
        B, N, K = toks.shape
        if B == 0:
            return torch.empty(0, N * self.config.hop_length, dtype=torch.float32, device=toks.device)
        nat = self._native_for(toks)
        toks = toks.to(torch.int64).contiguous()
        sig = torch.empty(B, N * self.config.hop_length, dtype=torch.float32, device=toks.device)
        with torch.cuda.device(nat.device):
            ws = nat.workspace(nat.lib.ac_decode_workspace_bytes(nat.h, B, N))
            _native.check(
                nat.lib.ac_decode(nat.h, _ptr(toks), B, N, K, _ptr(sig), _ptr(ws), ws.numel(), _stream()),
                nat.h, "ac_decode",
            )
        return sig

    # override
    def _toks_to_qfeats(self, toks, length):
        # toks: [B, N, K] -> [B, N, hidden]
        B, N, K = toks.shape
        if B == 0:
            return torch.empty(0, N, self.config.hidden_size, dtype=torch.float32, device=toks.device)
        nat = self._native_for(toks)
        toks = toks.to(torch.int64).contiguous()
        out = torch.empty(B, N, self.config.hidden_size, dtype=torch.float32, device=toks.device)
        with torch.cuda.device(nat.device):
            ws = nat.workspace(nat.lib.ac_quantizer_workspace_bytes(nat.h, B, N))
            _native.check(
                nat.lib.ac_dequantize_ws(nat.h, _ptr(toks), B, N, K, _ptr(out), _ptr(ws), ws.numel(), _stream()),
                nat.h, "ac_dequantize_ws",
            )
        return out

    # ---- streaming encode ------------------------------------------------------------------------
    def encode_stream(self, batch_size: int, device=None, *, resample: bool = False) -> "MimiEncodeStream":
        """A stateful signal -> tokens encoder for `batch_size` independent streams on `device` (default: the current cuda
        device).  Feed it with `push`; every push returns the tokens of the frames it completed (include/audiocodecs_amd.h
        ac_mimi_stream_*).  `resample=True`: the pushes are at `sample_rate` and go through a
        `ResampleStream` to the codec's rate first (close the stream with `finish`)."""
        if self.mode == "decode":
            raise ValueError("encode_stream needs the encoder: this Mimi was built with mode=\"decode\"")
        if self.sample_rate != self.config.sampling_rate and not resample:
            raise ValueError(
                f"encode_stream runs at the codec's own rate ({self.config.sampling_rate} Hz): streaming resampling from or to "
                f"sample_rate={self.sample_rate} is opt-in, pass resample=True"
            )
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"`batch_size` ({batch_size!r}) must be a positive int")
        self._check_num_codebooks()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return MimiEncodeStream(self, self._native_for(torch.empty(0, device=dev)), batch_size, bool(resample))

    # ---- streaming decode ------------------------------------------------------------------------
    def decode_stream(self, batch_size: int, device=None, *, resample: bool = False) -> "MimiDecodeStream":
        """A stateful tokens -> signal decoder for `batch_size` independent streams on `device` (default: the current cuda
        device).  Feed it with `push`; every push returns the samples of the frames it was given (include/audiocodecs_amd.h
        ac_mimi_stream_decode*).  `resample=True`: the samples come out at `sample_rate`, through a
        `ResampleStream` behind the decoder (`finish` returns its tail)."""
        if self.mode == "encode":
            raise ValueError("decode_stream needs the decoder: this Mimi was built with mode=\"encode\"")
        if self.sample_rate != self.config.sampling_rate and not resample:
            raise ValueError(
                f"decode_stream runs at the codec's own rate ({self.config.sampling_rate} Hz): streaming resampling from or to "
                f"sample_rate={self.sample_rate} is opt-in, pass resample=True"
            )
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"`batch_size` ({batch_size!r}) must be a positive int")
        self._check_num_codebooks()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return MimiDecodeStream(self, self._native_for(torch.empty(0, device=dev)), batch_size, bool(resample))

    # ---- session pools ---------------------------------------------------------------------------
    def _sessions_checks(self, what: str, capacity, device) -> _NativeMimi:
        need, lacks = ("encoder", "decode") if what.startswith("encode") else ("decoder", "encode")
        if self.mode == lacks:
            raise ValueError(f"{what} needs the {need}: this Mimi was built with mode=\"{lacks}\"")
        if self.sample_rate != self.config.sampling_rate:
            raise ValueError(
                f"{what} runs at the codec's own rate ({self.config.sampling_rate} Hz): streaming resampling from or to "
                f"sample_rate={self.sample_rate} is not available per slot"
            )
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError(f"`capacity` ({capacity!r}) must be a positive int")
        self._check_num_codebooks()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return self._native_for(torch.empty(0, device=dev))

    def encode_sessions(self, capacity: int, device=None) -> "MimiEncodeSessions":
        """A pool of up to `capacity` independent encode sessions on one stream state: sessions `open` and `close` at any time and
        `push(slots, sig)` serves any subset of them, each at its own position and with the bits of a lone `encode_stream(1)`
        (DESIGN.md section 8g).  Runs at the codec's own rate only."""
        return MimiEncodeSessions(self, self._sessions_checks("encode_sessions", capacity, device), capacity)

    def decode_sessions(self, capacity: int, device=None) -> "MimiDecodeSessions":
        """The decode side of `encode_sessions`: `push(slots, toks)` returns every listed session's samples."""
        return MimiDecodeSessions(self, self._sessions_checks("decode_sessions", capacity, device), capacity)

    # ---- measurement hook used by bench.py ------------------------------------------------------
    def profile_kernels(self, fn):
        nat = self._any_native()
        _native.check(nat.lib.ac_profile_begin(nat.h), nat.h, "ac_profile_begin")
        try:
            fn()
        finally:
            buf = (_native.AcKernelStat * 256)()
            n = nat.lib.ac_profile_end(nat.h, buf, 256)
        _native.check(n, nat.h, "ac_profile_end")
        return [(buf[i].name.decode(), buf[i].launches, buf[i].total_ms, buf[i].flops, buf[i].bytes) for i in range(n)]


def _boundary_resampler(codec, kind: str, batch_size: int, device, resample: bool):
    """resample=True at another rate than the codec's: the boundary's resampler, in front of the encoder or behind the decoder."""
    rate, own = int(codec.sample_rate), int(codec.config.sampling_rate)
    if not resample or rate == own:
        return None
    return ResampleStream(rate, own, batch_size, device) if kind == "encode" else ResampleStream(own, rate, batch_size, device)


_SHARED_PHASE = ("the slots of a resampling stream share one phase: a slot restarted alone would emit a different number of samples per "
                 "push than its neighbours (`streams` must be None)")


class MimiEncodeStream:
    """Streaming Mimi encode of `batch_size` streams (Mimi.encode_stream).  `push(sig)` takes [B, L] fp32 samples on the codec's
    device, any L >= 0, and returns the int64 tokens [B, n, K] of the n frames completed so far (n may be 0); a partial frame
    waits here until a later push completes it (`pending` samples, always below hop).  The tokens of a stream do not depend on
    how its signal was split into pushes, nor on the other streams.  The stream state and the workspace are device tensors owned
    by this object.

    With `resample=True` on a codec whose `sample_rate` is not the model's, `push` takes samples at `sample_rate`; they pass a
    `ResampleStream` (0.5 ms of added latency for 16 -> 24 kHz) and frames then count resampled samples.  `finish()` flushes the
    resampler's tail into the encoder and returns the tokens of any frame that completes; a trailing partial frame stays `pending`.
    After `finish` only `reset` is accepted, and single slots cannot be reset (they share the resampler's phase)."""

    MAX_POSITIONS = 1 << 24     # transformer positions per stream (fp32 RoPE angle)

    def __init__(self, codec: Mimi, nat: _NativeMimi, batch_size: int, resample: bool = False):
        self.codec = codec
        self._nat = nat
        self.batch_size = B = batch_size
        self.num_codebooks = codec.num_codebooks
        self.hop = codec.config.hop_length
        self.device = nat.device
        self._rs = _boundary_resampler(codec, "encode", B, self.device, resample)
        self._finished = False
        nbytes = nat.lib.ac_mimi_stream_state_bytes(nat.h, B)
        if nbytes == 0:
            raise _native.NativeError("ac_mimi_stream_state_bytes returned 0")
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self._ws = None
        self._pending = torch.empty(B, 0, dtype=torch.float32, device=self.device)
        self._frames = [0] * B
        self.reset()

    @property
    def pending(self) -> int:
        return int(self._pending.shape[1])

    def _call(self, rc, what):
        _native.check(rc, self._nat.h, what)

    @torch.no_grad()
    def reset(self, streams=None) -> None:
        """Start all streams afresh (dropping a pending partial frame), or only the listed slots (not while a partial frame is
        pending: its samples belong to every slot)."""
        nat, B = self._nat, self.batch_size
        mask = None
        if streams is not None:
            if self._rs is not None:
                raise ValueError(_SHARED_PHASE)
            idx = [streams] if isinstance(streams, int) else list(streams)
            if any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < B for i in idx):
                raise ValueError(f"`streams` ({streams!r}) must list slots in [0, {B})")
            if self.pending:
                raise ValueError(f"cannot reset single streams while {self.pending} samples of a partial frame are pending")
            m = torch.zeros(B, dtype=torch.uint8)
            m[idx] = 1
            mask = m.to(self.device)
            for i in idx:
                self._frames[i] = 0
        else:
            self._pending = self._pending[:, :0]
            self._frames = [0] * B
            self._finished = False
            if self._rs is not None:
                self._rs.reset()
        with torch.cuda.device(self.device):
            self._call(nat.lib.ac_mimi_stream_reset(nat.h, _ptr(self._state), self._state.numel(), B, _ptr(mask), _stream()),
                       "ac_mimi_stream_reset")

    @torch.no_grad()
    def push(self, sig: torch.Tensor) -> torch.Tensor:
        B, hop, K = self.batch_size, self.hop, self.num_codebooks
        if not isinstance(sig, torch.Tensor) or sig.dim() != 2 or sig.shape[0] != B:
            raise ValueError(f"push expects a [{B}, L] tensor, got {tuple(sig.shape) if isinstance(sig, torch.Tensor) else type(sig)}")
        if sig.dtype != torch.float32:
            raise ValueError(f"push expects float32 samples, got {sig.dtype}")
        if sig.device != self.device:
            raise ValueError(f"push expects samples on {self.device}, got {sig.device}")
        if self._finished:
            raise ValueError("push after finish: the stream is closed (call reset() first)")
        return self._take(self._resampled(sig, False) if self._rs is not None else sig)

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """Close the streams: the resampler's tail goes through the encoder; returns the tokens [B, n, K] of the frames it completes."""
        if self._finished:
            raise ValueError("finish after finish: the stream is closed (call reset() first)")
        toks = self._take(self._resampled(None, True) if self._rs is not None
                          else torch.empty(self.batch_size, 0, dtype=torch.float32, device=self.device))
        self._finished = True
        return toks

    def _resampled(self, sig, finish: bool) -> torch.Tensor:
        """The pending samples with the resampler's output for this push written straight behind them (one buffer, no second copy)."""
        rs, pend = self._rs, self.pending
        m = rs.out_len(0 if finish else sig.shape[1], finish)
        whole = torch.empty(self.batch_size, pend + m, dtype=torch.float32, device=self.device)
        if pend:
            whole[:, :pend].copy_(self._pending)
        if finish:
            rs.finish(out=whole[:, pend:])
        else:
            rs.push(sig, out=whole[:, pend:])
        self._pending = self._pending[:, :0]
        return whole

    def _take(self, sig: torch.Tensor) -> torch.Tensor:
        """Samples at the codec's rate: run the frames they complete, keep the rest pending."""
        B, hop, K = self.batch_size, self.hop, self.num_codebooks
        total = self.pending + sig.shape[1]
        n = total // hop
        if n == 0:
            self._pending = torch.cat([self._pending, sig], 1) if sig.shape[1] else self._pending
            return torch.empty(B, 0, K, dtype=torch.int64, device=self.device)
        if 2 * (max(self._frames) + n) > self.MAX_POSITIONS:
            raise ValueError(f"a stream would pass {self.MAX_POSITIONS} transformer positions: reset it first")
        whole = torch.cat([self._pending, sig], 1) if self.pending else sig
        chunk = whole[:, : n * hop].contiguous()
        nat = self._nat
        toks = torch.empty(B, n, K, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            need = nat.lib.ac_mimi_stream_workspace_bytes(nat.h, B, n)
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._call(nat.lib.ac_mimi_stream_encode(nat.h, _ptr(self._state), self._state.numel(), _ptr(chunk), B, n, K, _ptr(toks),
                                                     _ptr(self._ws), self._ws.numel(), _stream()), "ac_mimi_stream_encode")
        self._pending = whole[:, n * hop:].clone()
        self._frames = [f + n for f in self._frames]
        return toks


class MimiDecodeStream:
    """Streaming Mimi decode of `batch_size` streams (Mimi.decode_stream).  `push(toks)` takes [B, F, K] int64 tokens on the codec's
    device, K = the codec's `num_codebooks`, any F >= 0, and returns the [B, F * hop] fp32 samples of those frames at the codec's own
    rate.  The samples of a stream are those `toks_to_sig` gives on the stream's whole token sequence, for any number of frames, and
    do not depend on the other streams.  The stream state and the workspace are device tensors owned by this object.

    With `resample=True` on a codec whose `sample_rate` is not the model's, the samples pass a `ResampleStream` to `sample_rate` on
    their way out: a push returns what the resampler has completed (the count varies), `finish()` its tail, and everything together
    has the length `toks_to_sig` returns.  After `finish` only `reset` is accepted, and single slots cannot be reset (they share the
    resampler's phase)."""

    MAX_POSITIONS = 1 << 24     # transformer positions per stream (fp32 RoPE angle)

    def __init__(self, codec: Mimi, nat: _NativeMimi, batch_size: int, resample: bool = False):
        self.codec = codec
        self._nat = nat
        self.batch_size = B = batch_size
        self.num_codebooks = codec.num_codebooks
        self.hop = codec.config.hop_length
        self._stride = codec.config.resample_stride
        self.device = nat.device
        self._rs = _boundary_resampler(codec, "decode", B, self.device, resample)
        self._finished = False
        nbytes = nat.lib.ac_mimi_stream_decode_state_bytes(nat.h, B)
        if nbytes == 0:
            raise _native.NativeError("ac_mimi_stream_decode_state_bytes returned 0")
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self._ws = None
        self._frames = [0] * B
        self.reset()

    def _call(self, rc, what):
        _native.check(rc, self._nat.h, what)

    @torch.no_grad()
    def reset(self, streams=None) -> None:
        """Start all streams afresh, or only the listed slots."""
        nat, B = self._nat, self.batch_size
        mask = None
        if streams is not None:
            if self._rs is not None:
                raise ValueError(_SHARED_PHASE)
            idx = [streams] if isinstance(streams, int) and not isinstance(streams, bool) else list(streams)
            if any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < B for i in idx):
                raise ValueError(f"`streams` ({streams!r}) must list slots in [0, {B})")
            m = torch.zeros(B, dtype=torch.uint8)
            m[idx] = 1
            mask = m.to(self.device)
        with torch.cuda.device(self.device):
            self._call(nat.lib.ac_mimi_stream_decode_reset(nat.h, _ptr(self._state), self._state.numel(), B, _ptr(mask), _stream()),
                       "ac_mimi_stream_decode_reset")
        if streams is None:
            self._frames = [0] * B
            self._finished = False
            if self._rs is not None:
                self._rs.reset()
        else:
            for i in idx:
                self._frames[i] = 0

    @torch.no_grad()
    def push(self, toks: torch.Tensor) -> torch.Tensor:
        B, hop, K = self.batch_size, self.hop, self.num_codebooks
        if not isinstance(toks, torch.Tensor) or toks.dim() != 3 or toks.shape[0] != B or toks.shape[2] != K:
            raise ValueError(f"push expects a [{B}, F, {K}] tensor, got {tuple(toks.shape) if isinstance(toks, torch.Tensor) else type(toks)}")
        if toks.dtype != torch.int64:
            raise ValueError(f"push expects int64 tokens, got {toks.dtype}")
        if toks.device != self.device:
            raise ValueError(f"push expects tokens on {self.device}, got {toks.device}")
        if self._finished:
            raise ValueError("push after finish: the stream is closed (call reset() first)")
        sig = self._decode(toks)
        return self._rs.push(sig) if self._rs is not None else sig

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """Close the streams: the resampler's tail [B, m] (nothing without one)."""
        if self._finished:
            raise ValueError("finish after finish: the stream is closed (call reset() first)")
        self._finished = True
        if self._rs is not None:
            return self._rs.finish()
        return torch.empty(self.batch_size, 0, dtype=torch.float32, device=self.device)

    def _decode(self, toks: torch.Tensor) -> torch.Tensor:
        B, hop, K = self.batch_size, self.hop, self.num_codebooks
        F = toks.shape[1]
        if F == 0:
            return torch.empty(B, 0, dtype=torch.float32, device=self.device)
        if self._stride * (max(self._frames) + F) > self.MAX_POSITIONS:
            raise ValueError(f"a stream would pass {self.MAX_POSITIONS} transformer positions: reset it first")
        toks = toks.contiguous()
        nat = self._nat
        sig = torch.empty(B, F * hop, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            need = nat.lib.ac_mimi_stream_decode_workspace_bytes(nat.h, B, F)
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            self._call(nat.lib.ac_mimi_stream_decode(nat.h, _ptr(self._state), self._state.numel(), _ptr(toks), B, F, K, _ptr(sig),
                                                     _ptr(self._ws), self._ws.numel(), _stream()), "ac_mimi_stream_decode")
        self._frames = [f + F for f in self._frames]
        return sig


class _MimiSessions:
    """A pool of independent sessions on one Mimi stream state (include/audiocodecs_amd.h ac_mimi_stream_*_slots).

    The state holds `capacity` slots.  `open` hands out the lowest free one and restarts it alone (the masked reset of the lockstep
    stream); `push(slots, x)` runs any subset, row i of `x` belonging to `slots[i]`.  Partial frames wait per slot; Mimi pads with
    zeros, so a fresh slot runs its first whole frame at once (no warm-up hold, unlike the EnCodec pools).  The rows of a push that
    run the same number of frames share one native call, the groups going out in ascending F (sessions.plan_push, warmup = 1); a
    slot's bits are those of a lone stream fed the same pieces, whichever slot it sits in and whatever the others do."""

    MAX_POSITIONS = 1 << 24     # transformer positions per session (fp32 RoPE angle)
    _unit = 1          # units per frame in what a slot holds back: samples on the encode side, token frames on the decode side

    def __init__(self, codec: Mimi, nat: _NativeMimi, capacity: int, kind: str):
        self.codec = codec
        self._nat = nat
        self.capacity = capacity
        self.num_codebooks = codec.num_codebooks
        self.hop = codec.config.hop_length
        self._stride = codec.config.resample_stride      # transformer positions per frame
        self.device = nat.device
        L = nat.lib
        self._fns = {
            "encode": (L.ac_mimi_stream_state_bytes, L.ac_mimi_stream_reset, L.ac_mimi_stream_workspace_bytes, L.ac_mimi_stream_encode_slots),
            "decode": (L.ac_mimi_stream_decode_state_bytes, L.ac_mimi_stream_decode_reset, L.ac_mimi_stream_decode_workspace_bytes,
                       L.ac_mimi_stream_decode_slots),
        }[kind]
        self._kind = kind
        nbytes = self._fns[0](nat.h, capacity)
        if nbytes == 0:
            raise _native.NativeError(f"ac_mimi_stream_{'decode_' if kind == 'decode' else ''}state_bytes returned 0")
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self._ws = None
        self._is_open = [False] * capacity
        self._ran = [0] * capacity              # frames run since the slot was opened
        self._held = [self._empty()] * capacity  # what waits per slot: [m] samples (decode: nothing ever waits)
        self._reset(None)                       # the one whole reset: the header, and the handle's record of the address

    def _reset(self, mask) -> None:
        nat = self._nat
        with torch.cuda.device(self.device):
            _native.check(self._fns[1](nat.h, _ptr(self._state), self._state.numel(), self.capacity, _ptr(mask), _stream()), nat.h,
                          f"ac_mimi_stream_{'decode_' if self._kind == 'decode' else ''}reset")

    # -- the slots -----------------------------------------------------------------------------------------------------------------
    @property
    def active(self):
        """The open slots, ascending."""
        return [s for s in range(self.capacity) if self._is_open[s]]

    def _slot(self, slot) -> int:
        if isinstance(slot, bool) or not isinstance(slot, int) or not 0 <= slot < self.capacity:
            raise ValueError(f"slot {slot!r} is outside [0, {self.capacity})")
        if not self._is_open[slot]:
            raise ValueError(f"slot {slot} is not open")
        return slot

    def pending(self, slot: int) -> int:
        """Units of `slot` that have not run: samples on the encode side, token frames (always 0) on the decode side."""
        return int(self._held[self._slot(slot)].shape[0])

    def frames(self, slot: int) -> int:
        """Frames `slot` has run since it was opened."""
        return self._ran[self._slot(slot)]

    @torch.no_grad()
    def open(self) -> int:
        """Take the lowest free slot and restart it alone (the others keep running); ValueError when the pool is full."""
        free = [s for s in range(self.capacity) if not self._is_open[s]]
        if not free:
            raise ValueError(f"the pool is full: all {self.capacity} slots are open")
        slot = free[0]
        mask = torch.zeros(self.capacity, dtype=torch.uint8)
        mask[slot] = 1
        self._reset(mask.to(self.device))
        self._is_open[slot] = True
        self._ran[slot] = 0
        self._held[slot] = self._empty()
        return slot

    def close(self, slot: int) -> None:
        """Free `slot`, dropping the partial frame it holds."""
        slot = self._slot(slot)
        self._is_open[slot] = False
        self._held[slot] = self._empty()

    # -- a push --------------------------------------------------------------------------------------------------------------------
    def _check_push(self, slots, x):
        try:
            slots = list(slots)
        except TypeError:
            raise ValueError(f"push expects a sequence of slots, got {type(slots)}")
        for s in slots:
            self._slot(s)
        if len(set(slots)) != len(slots):
            raise ValueError(f"push: a slot is listed twice in {slots}")
        self._check_rows(len(slots), x)
        return slots

    def _run(self, slots, src: torch.Tensor, F: int, dst: torch.Tensor) -> None:
        nat, n = self._nat, len(slots)
        with torch.cuda.device(self.device):
            need = self._fns[2](nat.h, n, F)
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            host = (C.c_int * n)(*slots)
            dev = torch.tensor(slots, dtype=torch.int32, device=self.device)
            _native.check(self._fns[3](nat.h, _ptr(self._state), self._state.numel(), self.capacity, host, _ptr(dev), n, _ptr(src), F,
                                       self.num_codebooks, _ptr(dst), _ptr(self._ws), self._ws.numel(), _stream()), nat.h,
                          f"ac_mimi_stream_{self._kind}_slots")
        for s in slots:
            self._ran[s] += F

    @torch.no_grad()
    def push(self, slots, x: torch.Tensor):
        """Feed row i of `x` to `slots[i]` (n distinct open slots); returns n tensors, what each slot releases (possibly nothing)."""
        slots = self._check_push(slots, x)
        unit = self._unit
        plan = plan_push([int(self._held[s].shape[0]) for s in slots], [self._ran[s] for s in slots], [int(x.shape[1])] * len(slots), unit, 1)
        for F, rows in plan:
            for i in rows:
                if self._stride * (self._ran[slots[i]] + F) > self.MAX_POSITIONS:
                    raise ValueError(f"slot {slots[i]} would pass {self.MAX_POSITIONS} transformer positions: close it and open a new session")
        whole = [torch.cat([self._held[s], x[i]], 0) if self._held[s].shape[0] else x[i] for i, s in enumerate(slots)]
        out = [self._nothing() for _ in slots]
        for F, rows in plan:
            src = torch.stack([whole[i][: F * unit] for i in rows], 0).contiguous()
            dst = self._result(len(rows), F)
            self._run([slots[i] for i in rows], src, F, dst)
            for j, i in enumerate(rows):
                out[i] = dst[j]
                whole[i] = whole[i][F * unit:]
        for i, s in enumerate(slots):
            self._held[s] = whole[i].clone()
        return out


class MimiEncodeSessions(_MimiSessions):
    """A pool of encode sessions (Mimi.encode_sessions).  `push(slots, sig)`: `sig` is [n, L] fp32 on the codec's device, any
    L >= 0; returns n int64 tensors [f_i, K], the tokens of the frames each slot completes."""

    def __init__(self, codec: Mimi, nat: _NativeMimi, capacity: int):
        self._unit = codec.config.hop_length
        super().__init__(codec, nat, capacity, "encode")

    def _empty(self):
        return torch.empty(0, dtype=torch.float32, device=self.device)

    def _nothing(self):
        return torch.empty(0, self.num_codebooks, dtype=torch.int64, device=self.device)

    def _result(self, n, F):
        return torch.empty(n, F, self.num_codebooks, dtype=torch.int64, device=self.device)

    def _check_rows(self, n, sig):
        if not isinstance(sig, torch.Tensor) or sig.dim() != 2 or sig.shape[0] != n:
            raise ValueError(f"push expects a [{n}, L] tensor for {n} slots, got {tuple(sig.shape) if isinstance(sig, torch.Tensor) else type(sig)}")
        if sig.dtype != torch.float32:
            raise ValueError(f"push expects float32 samples, got {sig.dtype}")
        if sig.device != self.device:
            raise ValueError(f"push expects samples on {self.device}, got {sig.device}")


class MimiDecodeSessions(_MimiSessions):
    """A pool of decode sessions (Mimi.decode_sessions).  `push(slots, toks)`: `toks` is [n, F, K] int64 on the codec's device,
    K = the codec's `num_codebooks`, any F >= 0; returns n fp32 tensors [F * hop], the samples of each slot's frames."""

    def __init__(self, codec: Mimi, nat: _NativeMimi, capacity: int):
        super().__init__(codec, nat, capacity, "decode")

    def _empty(self):
        return torch.empty(0, self.num_codebooks, dtype=torch.int64, device=self.device)

    def _nothing(self):
        return torch.empty(0, dtype=torch.float32, device=self.device)

    def _result(self, n, F):
        return torch.empty(n, F * self.hop, dtype=torch.float32, device=self.device)

    def _check_rows(self, n, toks):
        K = self.num_codebooks
        if not isinstance(toks, torch.Tensor) or toks.dim() != 3 or toks.shape[0] != n or toks.shape[2] != K:
            raise ValueError(f"push expects a [{n}, F, {K}] tensor for {n} slots, got {tuple(toks.shape) if isinstance(toks, torch.Tensor) else type(toks)}")
        if toks.dtype != torch.int64:
            raise ValueError(f"push expects int64 tokens, got {toks.dtype}")
        if toks.device != self.device:
            raise ValueError(f"push expects tokens on {self.device}, got {toks.device}")
