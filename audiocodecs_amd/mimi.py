"""Mimi on MI355X -- host-side mirror of the reference wrapper `audiocodecs.Mimi`
(/root/reference/audiocodecs/mimi.py:25-156): same constructor arguments (`sample_rate`, `mode`,
`num_codebooks`, `latent`), attributes (`num_codebooks`, `vocab_size`, `latent`), method names, tensor
layouts and error behaviour.  The third-party `transformers.MimiModel` the reference calls
(mimi.py:45,105,115-119,139,146,153) is replaced by the gfx950 kernels behind the C ABI
(include/audiocodecs_amd.h, ac_mimi_create).  PyTorch is used for device memory and streams only.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _native
from .codec import Codec
from .config import MIMI_24KHZ, MimiConfig
from ._native import Handle, _ptr, _stream
from .sessions import SessionPool
from .streams import LockstepStream, StreamBackend, stream_checks

__all__ = ["Mimi", "MimiEncodeStream", "MimiDecodeStream", "MimiEncodeSessions", "MimiDecodeSessions"]


def _handle(cfg: MimiConfig, sd: Dict[str, torch.Tensor], device: torch.device, precision=None) -> Handle:
    c = _native.AcMimiConfig()
    for f in ("sampling_rate", "num_filters", "hidden_size", "kernel_size", "last_kernel_size", "residual_kernel_size",
              "compress", "codebook_size", "codebook_dim", "num_quantizers", "num_semantic_quantizers", "num_hidden_layers",
              "num_attention_heads", "head_dim", "intermediate_size", "sliding_window", "resample_stride", "rope_theta", "norm_eps"):
        setattr(c, f, getattr(cfg, f))
    c.num_ratios = len(cfg.upsampling_ratios)
    for i, r in enumerate(cfg.upsampling_ratios):
        c.upsampling_ratios[i] = r
    weights = {k: v for k, v in sd.items() if not k.endswith(".initialized")}    # (the codebooks' training flags)
    return Handle("ac_mimi_create", c, "is a gfx950 GPU visible?", weights, device, precision)


class Mimi(_native.HandleOwner, Codec):
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
        self._natives: Dict[int, Handle] = {}

    @staticmethod
    def _fetch_pretrained():
        try:
            from huggingface_hub import hf_hub_download
            from safetensors.torch import load_file
        except ImportError:
            raise ImportError("`pip install huggingface_hub safetensors` to fetch pretrained Mimi weights")
        return load_file(hf_hub_download("kyutai/mimi", "model.safetensors"))

    def _new_handle(self, device: torch.device) -> Handle:
        return _handle(self.config, self._sd, device, self.precision)

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

    # ---- streaming -------------------------------------------------------------------------------
    def _stream_checks(self, what: str, n, device, resample=False) -> Handle:
        return stream_checks(self, "Mimi", what, n, device, resample, self._check_num_codebooks)

    def encode_stream(self, batch_size: int, device=None, *, resample: bool = False) -> "MimiEncodeStream":
        """A stateful signal -> tokens encoder for `batch_size` independent streams on `device` (default: the current cuda
        device).  Feed it with `push`; every push returns the tokens of the frames it completed (include/audiocodecs_amd.h
        ac_mimi_stream_*).  `resample=True`: the pushes are at `sample_rate` and go through a
        `ResampleStream` to the codec's rate first (close the stream with `finish`)."""
        return MimiEncodeStream(self, self._stream_checks("encode_stream", batch_size, device, resample), batch_size, bool(resample))

    def decode_stream(self, batch_size: int, device=None, *, resample: bool = False) -> "MimiDecodeStream":
        """A stateful tokens -> signal decoder for `batch_size` independent streams on `device` (default: the current cuda
        device).  Feed it with `push`; every push returns the samples of the frames it was given (include/audiocodecs_amd.h
        ac_mimi_stream_decode*).  `resample=True`: the samples come out at `sample_rate`, through a
        `ResampleStream` behind the decoder (`finish` returns its tail)."""
        return MimiDecodeStream(self, self._stream_checks("decode_stream", batch_size, device, resample), batch_size, bool(resample))

    def encode_sessions(self, capacity: int, device=None, *, resample: bool = False) -> "MimiEncodeSessions":
        """A pool of up to `capacity` independent encode sessions on one stream state: sessions `open` and `close` at any time and
        `push(slots, sig)` serves any subset of them, each at its own position and with the bits of a lone `encode_stream(1)`
        (DESIGN.md section 8g).  `resample=True`: the pushes are at `sample_rate` and pass a `ResampleSlots` to the codec's
        rate first, every session at its own phase (section 8h; close a session's signal with `finish(slot)`)."""
        return MimiEncodeSessions(self, self._stream_checks("encode_sessions", capacity, device, resample), capacity, bool(resample))

    def decode_sessions(self, capacity: int, device=None, *, resample: bool = False) -> "MimiDecodeSessions":
        """The decode side of `encode_sessions`: `push(slots, toks)` returns every listed session's samples.  `resample=True`: they
        come out at `sample_rate`, through a `ResampleSlots` behind the decoder (`finish(slot)` returns a session's tail)."""
        return MimiDecodeSessions(self, self._stream_checks("decode_sessions", capacity, device, resample), capacity, bool(resample))


class _OnMimi:
    """The Mimi side of the four classes below: their backend and the position limit.  Mimi pads with zeros, so a fresh stream runs
    its first whole frame at once (warm-up 1: no hold, unlike EnCodec), and a slot restarts alone through the masked reset; the
    transformers advance `resample_stride` positions per frame."""

    MAX_POSITIONS = 1 << 24     # transformer positions per stream or session (fp32 RoPE angle)

    def __init__(self, codec: Mimi, nat: Handle, n: int, *resample):
        be = StreamBackend(nat, "ac_mimi_stream", self._kind, codec.config.hop_length, stride=codec.config.resample_stride)
        super().__init__(codec, be, n, codec.num_codebooks, *resample)


class MimiEncodeStream(_OnMimi, LockstepStream):
    """Streaming Mimi encode of `batch_size` streams (Mimi.encode_stream).  `push(sig)` takes [B, L] fp32 samples on the codec's
    device, any L >= 0, and returns the int64 tokens [B, n, K] of the n frames completed so far (n may be 0); a partial frame
    waits here until a later push completes it (`pending` samples, always below hop).  The tokens of a stream do not depend on
    how its signal was split into pushes, nor on the other streams.  The stream state and the workspace are device tensors owned
    by this object.  `reset()` starts all streams afresh (dropping a pending partial frame), `reset(streams)` only the listed slots
    (not while a partial frame is pending: its samples belong to every slot).

    With `resample=True` on a codec whose `sample_rate` is not the model's, `push` takes samples at `sample_rate`; they pass a
    `ResampleStream` (0.5 ms of added latency for 16 -> 24 kHz) and frames then count resampled samples.  `finish()` flushes the
    resampler's tail into the encoder and returns the tokens of any frame that completes; a trailing partial frame stays `pending`.
    After `finish` only `reset` is accepted, and single slots cannot be reset (they share the resampler's phase)."""

    _kind = "encode"
    pending = LockstepStream._waiting


class MimiDecodeStream(_OnMimi, LockstepStream):
    """Streaming Mimi decode of `batch_size` streams (Mimi.decode_stream).  `push(toks)` takes [B, F, K] int64 tokens on the codec's
    device, K = the codec's `num_codebooks`, any F >= 0, and returns the [B, F * hop] fp32 samples of those frames at the codec's own
    rate.  The samples of a stream are those `toks_to_sig` gives on the stream's whole token sequence, for any number of frames, and
    do not depend on the other streams.  The stream state and the workspace are device tensors owned by this object.  `reset()` starts
    all streams afresh, `reset(streams)` only the listed slots.

    With `resample=True` on a codec whose `sample_rate` is not the model's, the samples pass a `ResampleStream` to `sample_rate` on
    their way out: a push returns what the resampler has completed (the count varies), `finish()` its tail, and everything together
    has the length `toks_to_sig` returns.  After `finish` only `reset` is accepted, and single slots cannot be reset (they share the
    resampler's phase)."""

    _kind = "decode"
    pending_frames = LockstepStream._waiting      # always 0: nothing is held back


class MimiEncodeSessions(_OnMimi, SessionPool):
    """A pool of encode sessions on one Mimi stream state (Mimi.encode_sessions; include/audiocodecs_amd.h ac_mimi_stream_*_slots).
    `push(slots, sig)`: `sig` is [n, L] fp32 on the codec's device, any L >= 0; returns n int64 tensors [f_i, K], the tokens of the
    frames each slot completes.  Partial frames wait per slot; there is no warm-up hold.  With `resample=True` on a codec at
    another rate, `sig` is at `sample_rate` and passes a `ResampleSlots` first, every slot at its own phase: frames, `pending` and
    the hold count resampled samples; `finish(slot)` flushes that slot's resampler and returns the tokens of any frame it completes,
    after which the slot accepts only `close`."""

    _kind = "encode"


class MimiDecodeSessions(_OnMimi, SessionPool):
    """A pool of decode sessions (Mimi.decode_sessions).  `push(slots, toks)`: `toks` is [n, F, K] int64 on the codec's device,
    K = the codec's `num_codebooks`, any F >= 0; returns n fp32 tensors [F * hop], the samples of each slot's frames.  With `resample=True`
    on a codec at another rate the samples pass a `ResampleSlots` to `sample_rate` on their way out: a push returns what each slot's
    resampler completed, `finish(slot)` its tail (`toks_to_sig`'s length in all), after which the slot accepts only `close`."""

    _kind = "decode"
