"""EnCodec on MI355X -- host-side mirror of the reference wrapper `audiocodecs.Encodec`
(/root/reference/audiocodecs/encodec.py:30-149): same constructor arguments, attributes
(`num_codebooks`, `vocab_size`, `bandwidth`), method names, tensor layouts and error behaviour.
The third-party `transformers.EncodecModel` the reference calls (encodec.py:51,90,116,125,139,147)
is replaced by the hand-written gfx950 kernels behind the C ABI in include/audiocodecs_amd.h.
PyTorch is used here only for device memory, streams and one-time weight-norm folding.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _native, checkpoint
from ._native import Handle, _ptr, _stream  # noqa: F401  (_ptr and _stream stay importable from here: the tests' raw-ABI cases do)
from .codec import Codec
from .config import ENCODEC_24KHZ, VOCOS_ENCODEC_24KHZ, EncodecConfig, VocosConfig
from .sessions import SessionPool
from .streams import LockstepStream, StreamBackend, stream_checks

__all__ = ["Encodec", "EncodecEncodeStream", "EncodecDecodeStream", "EncodecEncodeSessions", "EncodecDecodeSessions"]


def _handle(cfg: EncodecConfig, folded: Dict[str, torch.Tensor], device: torch.device, precision=None) -> Handle:
    c = _native.AcConfig()
    for f in ("sampling_rate", "num_filters", "hidden_size", "kernel_size", "last_kernel_size", "residual_kernel_size", "compress",
              "num_lstm_layers", "codebook_size", "num_quantizers"):
        setattr(c, f, getattr(cfg, f))
    c.num_ratios = len(cfg.upsampling_ratios)
    for i, r in enumerate(cfg.upsampling_ratios):
        c.upsampling_ratios[i] = r
    return Handle("ac_create", c, "is a gfx950 GPU visible?", folded, device, precision)


def _vocos_handle(cfg: VocosConfig, bandwidth_id: int, sd: Dict[str, torch.Tensor], device: torch.device, precision=None) -> Handle:
    c = _native.AcVocosConfig()
    for f in ("input_channels", "codebook_size", "max_codebooks", "backbone_dim", "intermediate_dim", "num_layers", "adanorm_num_embeddings",
              "n_fft", "hop_length"):
        setattr(c, f, getattr(cfg, f))
    c.bandwidth_id = bandwidth_id
    return Handle("ac_vocos_create", c, "is a gfx950 GPU visible?", sd, device, precision)


class Encodec(_native.HandleOwner, Codec):
    _accepts_none_length = True
    _graph_capable = False        # codec.py: the persistent LSTM launch is not replayable from a hipGraph

    def __init__(
        self,
        sample_rate,
        orig_sample_rate=24000,
        mode="reconstruct",
        num_codebooks=8,
        use_vocos=False,
        *,
        state_dict: Optional[Dict[str, torch.Tensor]] = None,
        config: EncodecConfig = ENCODEC_24KHZ,
        precision: Optional[str] = None,
        strict: bool = False,
        graph: bool = False,
        vocos_state_dict: Optional[Dict[str, torch.Tensor]] = None,
        vocos_config: VocosConfig = VOCOS_ENCODEC_24KHZ,
    ):
        """`state_dict`: an HF-format EncodecModel state dict (keys of SURVEY.md Appendix A.3, e.g.
        `safetensors.torch.load_file(model.safetensors)` of facebook/encodec_24khz, or
        `checkpoint.synthetic_state_dict(cfg, seed)`).  When omitted the pretrained checkpoint is
        fetched through huggingface_hub like the reference does (needs network or a warm cache).
        `precision`: None / "fp32" = fp32 fidelity on the fp16 matrix pipe (split16: the parity arithmetic, default);
        "fp32_exact" = exact fp32 products (include/audiocodecs_amd.h ac_set_precision).
        `use_vocos=True` (encodec.py:53-66): in the decoding modes `toks_to_sig` runs the Vocos decoder instead of the SEANet one, whose
        weights are then never packed or uploaded (`mode="encode"` keeps no Vocos at all, :67-69).  `vocos_state_dict`: the state dict of
        charactr/vocos-encodec-24khz (`torch.load(pytorch_model.bin)`, or `checkpoint.synthetic_vocos_state_dict(vocos_config, seed)`);
        when omitted it is fetched through huggingface_hub like the reference does.  PARITY UNPINNED: the reference's `vocos` package is
        not on disk, the path is held to a restatement of the published Vocos 0.1.0 modules (tests/vocos_ref.py).
        With Vocos, `graph=True` replays `toks_to_sig` (no LSTM on that path); `sig_to_toks` still runs eagerly."""
        super().__init__(sample_rate, orig_sample_rate, mode)
        self.strict = bool(strict)   # codec.py: poll the handle after every call
        self.graph = bool(graph)     # codec.py: replay one hipGraph per (call, shape)
        self.precision = _native.check_precision(precision)
        if config.sampling_rate != orig_sample_rate:
            raise ValueError(f"config.sampling_rate ({config.sampling_rate}) != orig_sample_rate ({orig_sample_rate})")
        self.num_codebooks = num_codebooks
        self.use_vocos = bool(use_vocos)
        self.vocab_size = config.codebook_size
        self.config = config
        self.bandwidth = (num_codebooks * 75) / 100  # encodec.py:50
        if state_dict is None:
            state_dict = self._fetch_pretrained(int(orig_sample_rate / 1000))
        self._folded = checkpoint.fold_weight_norm(state_dict)
        # encodec.py:67-71: the half of the model the mode never runs is dropped (here: never packed or uploaded)
        if mode == "encode":
            self._folded = {k: v for k, v in self._folded.items() if not k.startswith("decoder.")}
        elif mode == "decode":
            self._folded = {k: v for k, v in self._folded.items() if not k.startswith("encoder.")}
        self._natives: Dict[int, Handle] = {}
        # encodec.py:53-69: with use_vocos a decoding mode swaps the SEANet decoder for Vocos (the quantizer stays: embs, toks_to_qfeats)
        self._vocos_sd = None
        self._vocos_natives: Dict[int, Handle] = {}
        self.vocos_config = vocos_config
        if self.use_vocos and mode != "encode":
            if vocos_config.hop_length != config.hop_length or vocos_config.input_channels != config.hidden_size or vocos_config.codebook_size != config.codebook_size:
                raise ValueError("vocos_config does not fit config: hop_length, input_channels == hidden_size and codebook_size must agree")
            if vocos_state_dict is None:
                vocos_state_dict = self._fetch_pretrained_vocos(int(orig_sample_rate / 1000))
            keep = ("feature_extractor.codebook_weights", "backbone.", "head.")     # (upstream re-attaches feature_extractor.encodec.* at load time)
            self._vocos_sd = {k: v for k, v in vocos_state_dict.items() if k.startswith(keep)}
            self._folded = {k: v for k, v in self._folded.items() if not k.startswith("decoder.")}

    @staticmethod
    def _fetch_pretrained(tag: int):
        try:
            from huggingface_hub import hf_hub_download
            from safetensors.torch import load_file
        except ImportError:
            raise ImportError("`pip install huggingface_hub safetensors` to fetch pretrained EnCodec weights")
        return load_file(hf_hub_download(f"facebook/encodec_{tag}khz", "model.safetensors"))

    @staticmethod
    def _fetch_pretrained_vocos(tag: int):
        try:
            from huggingface_hub import hf_hub_download
        except ImportError:
            raise ImportError("`pip install huggingface_hub` to fetch pretrained Vocos weights")
        return torch.load(hf_hub_download(f"charactr/vocos-encodec-{tag}khz", "pytorch_model.bin"), map_location="cpu")

    def _new_handle(self, device: torch.device) -> Handle:
        return _handle(self.config, self._folded, device, self.precision)

    def _vocos_bandwidth_id(self) -> int:
        """encodec.py:56: `[1.5, 3.0, 6.0, 12.0].index(self.bandwidth)` -- a ValueError at the call for any other `num_codebooks`."""
        return list(self.vocos_config.bandwidths).index(self.bandwidth)

    def _vocos_for(self, t: torch.Tensor, bandwidth_id: int) -> Handle:
        if not t.is_cuda:
            raise _native.NativeError("audiocodecs_amd runs on MI355X only: move the input to a cuda device (there is deliberately no CPU fallback)")
        idx = t.device.index
        if idx not in self._vocos_natives:
            self._vocos_natives[idx] = _vocos_handle(self.vocos_config, bandwidth_id, self._vocos_sd, t.device, self.precision)
        return self._vocos_natives[idx]

    def _handles(self):
        return list(self._natives.values()) + list(self._vocos_natives.values())

    def _profiled_handles(self):
        return [self._any_native()] + list(self._vocos_natives.values())

    def _graph_ok(self, name) -> bool:
        return name == "toks_to_sig" and self._vocos_sd is not None      # the Vocos decode has no LSTM: replayable

    def _num_quantizers(self) -> int:
        """[HF] modeling_encodec.py:564-567 rejects bandwidths outside config.target_bandwidths,
        then :416-422 maps the bandwidth to a stage count."""
        if self.bandwidth not in self.config.target_bandwidths:
            raise ValueError(
                f"This model doesn't support the bandwidth {self.bandwidth}. "
                f"Select one of {list(self.config.target_bandwidths)}."
            )
        return self.config.num_quantizers_for_bandwidth(self.bandwidth)

    def _check_length(self, sig, length):
        """encodec.py:84-89 builds a [B, max_len] mask with max_len = int(max(T*length)); the model
        then multiplies it with the [B,1,T] input, which only works when max_len == T."""
        if length is None:
            return None
        length = length.to(device=sig.device, dtype=torch.float32).contiguous()
        max_len = int((sig.shape[-1] * length).max().long().item())
        if max_len != sig.shape[-1]:
            raise RuntimeError(
                f"The size of the padding mask ({max_len}) must match the signal length ({sig.shape[-1]}): "
                "relative lengths must have a maximum of 1.0"
            )
        return length

    # override
    @torch.no_grad()
    def embs(self):
        nat = self._any_native()
        out = torch.empty(self.num_codebooks, self.vocab_size, self.config.hidden_size, device=nat.device)
        with torch.cuda.device(nat.device):
            _native.check(nat.lib.ac_embs(nat.h, self.num_codebooks, _ptr(out), _stream()), nat.h, "ac_embs")
        return out  # [K, C, H]

    # override
    def _sig_to_toks(self, sig, length):
        # sig: [B, T]
        K = self._num_quantizers()
        B, T = sig.shape
        N = self.config.num_frames(T)
        if B == 0:   # an empty shard (sharding.shard_bounds): nothing to run, the library is not called
            return torch.empty(0, N, K, dtype=torch.int64, device=sig.device)
        nat = self._native_for(sig)
        sig = sig.to(torch.float32).contiguous()
        length = self._check_length(sig, length)
        toks = torch.empty(B, N, K, dtype=torch.int64, device=sig.device)
        with torch.cuda.device(nat.device):
            nbytes = nat.lib.ac_encode_workspace_bytes(nat.h, B, T)
            ws = nat.workspace(nbytes)
            _native.check(
                nat.lib.ac_encode(nat.h, _ptr(sig), _ptr(length), B, T, K, _ptr(toks), _ptr(ws), ws.numel(), _stream()),
                nat.h, "ac_encode",
            )
        return toks  # [B, N, K]

    # override
    def _sig_to_feats(self, sig, length):
        # sig: [B, T] -> [B, N, H].  The reference masks here only when config.normalize
        # (encodec.py:107-112): never for the 24 kHz model, so `length` is ignored.
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
        toks = self._sig_to_toks(sig, length)
        return self._toks_to_qfeats(toks, length)

    # override
    def _toks_to_sig(self, toks, length):
        # toks: [B, N, K] -> [B, N*hop]
        vocos = self._vocos_sd is not None
        bw_id = self._vocos_bandwidth_id() if vocos else None      # (raises before any device or shape check, like the reference)
        B, N, K = toks.shape
        if vocos and not 1 <= K <= self.vocos_config.max_codebooks:
            raise ValueError(f"Vocos decodes 1 to {self.vocos_config.max_codebooks} codebooks, the tokens have {K}")
        if B == 0:
            return torch.empty(0, N * self.config.hop_length, dtype=torch.float32, device=toks.device)
        nat = self._vocos_for(toks, bw_id) if vocos else self._native_for(toks)
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
        # toks: [B, N, K] -> [B, N, H]
        B, N, K = toks.shape
        if B == 0:
            return torch.empty(0, N, self.config.hidden_size, dtype=torch.float32, device=toks.device)
        nat = self._native_for(toks)
        toks = toks.to(torch.int64).contiguous()
        out = torch.empty(B, N, self.config.hidden_size, dtype=torch.float32, device=toks.device)
        with torch.cuda.device(nat.device):
            _native.check(nat.lib.ac_dequantize(nat.h, _ptr(toks), B, N, K, _ptr(out), _stream()), nat.h, "ac_dequantize")
        return out

    # ---- streaming -------------------------------------------------------------------------------
    def _stream_checks(self, what: str, n, device, resample=False) -> Handle:
        return stream_checks(self, "Encodec", what, n, device, resample, self._num_quantizers)

    def encode_stream(self, batch_size: int, device=None, *, resample: bool = False) -> "EncodecEncodeStream":
        """A stateful signal -> tokens encoder for `batch_size` independent streams on `device` (default: the current cuda
        device).  Feed it with `push`; after the start-up hold of `WARMUP_FRAMES` frames every push returns the tokens of the
        frames it completed (include/audiocodecs_amd.h ac_encodec_stream_*).  `resample=True`: the
        pushes are at `sample_rate` and go through a `ResampleStream` to the codec's rate first (close the stream with `finish`)."""
        return EncodecEncodeStream(self, self._stream_checks("encode_stream", batch_size, device, resample), batch_size, bool(resample))

    def decode_stream(self, batch_size: int, device=None, *, resample: bool = False) -> "EncodecDecodeStream":
        """A stateful tokens -> signal decoder for `batch_size` independent streams on `device` (default: the current cuda
        device).  Feed it with `push`; after the start-up hold of `WARMUP_FRAMES` frames every push returns the samples of the
        frames it was given (include/audiocodecs_amd.h ac_encodec_stream_decode*).  `resample=True`:
        the samples come out at `sample_rate`, through a `ResampleStream` behind the decoder (`finish` returns its tail)."""
        return EncodecDecodeStream(self, self._stream_checks("decode_stream", batch_size, device, resample), batch_size, bool(resample))

    def encode_sessions(self, capacity: int, device=None, *, resample: bool = False) -> "EncodecEncodeSessions":
        """A pool of up to `capacity` independent encode sessions on one stream state: sessions `open` and `close` at any time and
        `push(slots, sig)` serves any subset of them, each with the warm-up hold and the bits of a lone `encode_stream(1)`
        (DESIGN.md section 8f).  `resample=True`: the pushes are at `sample_rate` and pass a `ResampleSlots` to the codec's
        rate first, every session at its own phase (section 8h; close a session's signal with `finish(slot)`)."""
        return EncodecEncodeSessions(self, self._stream_checks("encode_sessions", capacity, device, resample), capacity, bool(resample))

    def decode_sessions(self, capacity: int, device=None, *, resample: bool = False) -> "EncodecDecodeSessions":
        """The decode side of `encode_sessions`: `push(slots, toks)` returns every listed session's samples.  `resample=True`: they
        come out at `sample_rate`, through a `ResampleSlots` behind the decoder (`finish(slot)` returns a session's tail)."""
        return EncodecDecodeSessions(self, self._stream_checks("decode_sessions", capacity, device, resample), capacity, bool(resample))


class _EncodecBackend(StreamBackend):
    """EnCodec pads every causal conv by REFLECTION, so the first rows of a clip see a mirror image of the rows that follow them.  A
    stream can reproduce that only once those rows are there: it holds back its first `WARMUP_FRAMES` = max(kernel_size,
    last_kernel_size) frames (7 frames = 93 ms at 75 frames/s) and runs them as one push.  With fewer the reference itself switches
    to its small-input padding rule and the one-shot result differs (tests/test_encodec_stream_oracle.py): the hold is the
    reference's padding, not a choice of this library.  Pool slots restart through the slot-list call (the LSTM state goes with them)."""

    reset_together = ("EnCodec streams reset together: a slot restarted alone would sit in its warm-up hold while the others run "
                      "(`streams` must be None)")

    def __init__(self, cfg: EncodecConfig, nat: Handle, kind: str):
        super().__init__(nat, "ac_encodec_stream", kind, cfg.hop_length, warmup=max(cfg.kernel_size, cfg.last_kernel_size))
        self._who["reset"] = f"ac_encodec_stream_{kind}_reset"
        self._reset_slots = getattr(nat.lib, f"ac_encodec_stream_{'decode_' if kind == 'decode' else ''}reset_slots")

    def restart_slots(self, state, cap, slots):
        nat, n = self._nat, len(slots)
        with torch.cuda.device(self.device):
            host = (C.c_int * n)(*slots)
            dev = torch.tensor(list(slots), dtype=torch.int32, device=self.device)
            _native.check(self._reset_slots(nat.h, _ptr(state), state.numel(), cap, host, _ptr(dev), n, _stream()), nat.h,
                          self._who["reset"] + "_slots")


class _OnEncodec:
    """The EnCodec side of the four classes below: their backend, the stage count and `WARMUP_FRAMES`."""

    def __init__(self, codec: Encodec, nat: Handle, n: int, *resample):
        be = _EncodecBackend(codec.config, nat, self._kind)
        self.WARMUP_FRAMES = be.warmup
        super().__init__(codec, be, n, codec._num_quantizers(), *resample)


class EncodecEncodeStream(_OnEncodec, LockstepStream):
    """Streaming EnCodec encode of `batch_size` streams (Encodec.encode_stream).  `push(sig)` takes [B, L] fp32 samples on the
    codec's device, any L >= 0, and returns the int64 tokens [B, n, K] of the frames it releases (n may be 0).  Samples that do not
    fill a frame wait here (`pending` samples).  A fresh stream releases nothing until `WARMUP_FRAMES` whole frames are in (the
    reference's reflect padding: 93 ms); the push that crosses that mark returns all frames completed so far, and from then on every
    frame comes out in the push that completes it.  The tokens of a stream are those `sig_to_toks` gives on its whole signal (up to
    near-ties: scales are taken per push), however it was split into pushes and whatever the other streams carry.  The stream state
    and the workspace are device tensors owned by this object.  `reset()` starts all streams afresh (`streams` must be None).

    With `resample=True` on a codec whose `sample_rate` is not the model's, `push` takes samples at `sample_rate`; they pass a
    `ResampleStream` (0.5 ms of added latency for 16 -> 24 kHz) and the frame and warm-up rules above then count resampled samples.
    `finish()` flushes the resampler's tail into the encoder and returns the tokens of any frame that completes; a trailing partial
    frame stays `pending`.  After `finish` only `reset` is accepted."""

    _kind = "encode"
    pending = LockstepStream._waiting
    frames = property(lambda self: self._frames[0], doc="Frames run so far (the same for every slot).")


class EncodecDecodeStream(_OnEncodec, LockstepStream):
    """Streaming EnCodec decode of `batch_size` streams (Encodec.decode_stream).  `push(toks)` takes [B, F, K] int64 tokens on the
    codec's device, K = the codec's stage count, any F >= 0, and returns [B, n * hop] fp32 samples.  A fresh stream holds its first
    tokens back (`pending_frames`) until `WARMUP_FRAMES` frames are in (the reference's reflect padding), returns the samples of all
    of them with the push that crosses that mark, and F * hop samples per push from then on.  The samples of a stream are those
    `toks_to_sig` gives on its whole token sequence (up to rounding), whatever the other streams carry.  The stream state and the
    workspace are device tensors owned by this object.  `reset()` starts all streams afresh (`streams` must be None).

    With `resample=True` on a codec whose `sample_rate` is not the model's, the samples pass a `ResampleStream` to `sample_rate` on
    their way out: a push returns what the resampler has completed (the count varies), `finish()` its tail, and everything together
    has the length `toks_to_sig` returns.  After `finish` only `reset` is accepted."""

    _kind = "decode"
    pending_frames = LockstepStream._waiting
    frames = EncodecEncodeStream.frames


class EncodecEncodeSessions(_OnEncodec, SessionPool):
    """A pool of encode sessions on one EnCodec stream state (Encodec.encode_sessions; include/audiocodecs_amd.h
    ac_encodec_stream_*_slots).  `push(slots, sig)`: `sig` is [n, L] fp32 on the codec's device, any L >= 0; returns n int64 tensors
    [f_i, K], the tokens of the frames each slot releases.  A fresh slot holds until `WARMUP_FRAMES` whole frames are in.  With `resample=True` on a codec at
    another rate, `sig` is at `sample_rate` and passes a `ResampleSlots` first, every slot at its own phase: frames, `pending` and
    the hold count resampled samples; `finish(slot)` flushes that slot's resampler and returns the tokens of any frame it completes,
    after which the slot accepts only `close`."""

    _kind = "encode"


class EncodecDecodeSessions(_OnEncodec, SessionPool):
    """A pool of decode sessions (Encodec.decode_sessions).  `push(slots, toks)`: `toks` is [n, F, K] int64 on the codec's device,
    K = the codec's stage count, any F >= 0; returns n fp32 tensors [f_i * hop], the samples of the frames each slot releases.  With `resample=True`
    on a codec at another rate the samples pass a `ResampleSlots` to `sample_rate` on their way out: a push returns what each slot's
    resampler completed, `finish(slot)` its tail (`toks_to_sig`'s length in all), after which the slot accepts only `close`."""

    _kind = "decode"
