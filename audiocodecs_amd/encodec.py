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
from .codec import Codec
from .config import ENCODEC_24KHZ, EncodecConfig
from .resample import ResampleStream
from .sessions import plan_push

__all__ = ["Encodec", "EncodecEncodeStream", "EncodecDecodeStream", "EncodecEncodeSessions", "EncodecDecodeSessions"]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Native:
    """One ac_handle: weights on one GPU + a grow-only workspace tensor."""

    def __init__(self, cfg: EncodecConfig, folded: Dict[str, torch.Tensor], device: torch.device, precision=None):
        self.lib = _native.lib()
        c = _native.AcConfig()
        c.struct_size = C.sizeof(_native.AcConfig)
        c.sampling_rate = cfg.sampling_rate
        c.num_filters = cfg.num_filters
        c.hidden_size = cfg.hidden_size
        c.num_ratios = len(cfg.upsampling_ratios)
        for i, r in enumerate(cfg.upsampling_ratios):
            c.upsampling_ratios[i] = r
        c.kernel_size = cfg.kernel_size
        c.last_kernel_size = cfg.last_kernel_size
        c.residual_kernel_size = cfg.residual_kernel_size
        c.compress = cfg.compress
        c.num_lstm_layers = cfg.num_lstm_layers
        c.codebook_size = cfg.codebook_size
        c.num_quantizers = cfg.num_quantizers
        c.device = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", c.device)
        self.h = C.c_void_p()
        rc = self.lib.ac_create(C.byref(c), C.byref(self.h))
        if rc < 0:
            raise _native.NativeError(f"ac_create failed with code {rc} (is a gfx950 GPU visible?)")
        _native.set_precision(self.lib, self.h, precision)
        for name, t in folded.items():
            if not t.is_floating_point():
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
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
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


class Encodec(Codec):
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
    ):
        """`state_dict`: an HF-format EncodecModel state dict (keys of SURVEY.md Appendix A.3, e.g.
        `safetensors.torch.load_file(model.safetensors)` of facebook/encodec_24khz, or
        `checkpoint.synthetic_state_dict(cfg, seed)`).  When omitted the pretrained checkpoint is
        fetched through huggingface_hub like the reference does (needs network or a warm cache).
        `precision`: None / "fp32" = fp32 fidelity on the fp16 matrix pipe (split16: the parity arithmetic, default);
        "fp32_exact" = exact fp32 products (include/audiocodecs_amd.h ac_set_precision)."""
        super().__init__(sample_rate, orig_sample_rate, mode)
        self.strict = bool(strict)   # codec.py: poll the handle after every call
        self.graph = bool(graph)     # codec.py: replay one hipGraph per (call, shape)
        self.precision = _native.check_precision(precision)
        if use_vocos:
            raise NotImplementedError("the Vocos decoder variant (encodec.py:53-66) is outside the MI355X path")
        if config.sampling_rate != orig_sample_rate:
            raise ValueError(f"config.sampling_rate ({config.sampling_rate}) != orig_sample_rate ({orig_sample_rate})")
        self.num_codebooks = num_codebooks
        self.use_vocos = use_vocos
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
        self._natives: Dict[int, _Native] = {}

    @staticmethod
    def _fetch_pretrained(tag: int):
        try:
            from huggingface_hub import hf_hub_download
            from safetensors.torch import load_file
        except ImportError:
            raise ImportError("`pip install huggingface_hub safetensors` to fetch pretrained EnCodec weights")
        return load_file(hf_hub_download(f"facebook/encodec_{tag}khz", "model.safetensors"))

    # ------------------------------------------------------------------------------------------
    def _native_for(self, t: torch.Tensor) -> _Native:
        if not t.is_cuda:
            raise _native.NativeError(
                "audiocodecs_amd runs on MI355X only: move the input to a cuda device "
                "(there is deliberately no CPU fallback)"
            )
        idx = t.device.index
        if idx not in self._natives:
            self._natives[idx] = _Native(self.config, self._folded, t.device, self.precision)
        return self._natives[idx]

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
        dev = next(iter(self._natives.values())).device if self._natives else torch.device("cuda", torch.cuda.current_device())
        nat = self._native_for(torch.empty(0, device=dev))
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
    def _stream_checks(self, what: str, batch_size, device, resample=False) -> _Native:
        need, lacks = ("encoder", "decode") if what.startswith("encode") else ("decoder", "encode")
        pool = what.endswith("sessions")
        if self.mode == lacks:
            raise ValueError(f"{what} needs the {need}: this Encodec was built with mode=\"{lacks}\"")
        if self.sample_rate != self.config.sampling_rate and not resample:
            raise ValueError(
                f"{what} runs at the codec's own rate ({self.config.sampling_rate} Hz): streaming resampling from or to "
                f"sample_rate={self.sample_rate} is " + ("not available per slot" if pool else "opt-in, pass resample=True")
            )
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"`{'capacity' if pool else 'batch_size'}` ({batch_size!r}) must be a positive int")
        self._num_quantizers()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        return self._native_for(torch.empty(0, device=dev))

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

    def encode_sessions(self, capacity: int, device=None) -> "EncodecEncodeSessions":
        """A pool of up to `capacity` independent encode sessions on one stream state: sessions `open` and `close` at any time and
        `push(slots, sig)` serves any subset of them, each with the warm-up hold and the bits of a lone `encode_stream(1)`
        (DESIGN.md section 8f).  Runs at the codec's own rate only."""
        return EncodecEncodeSessions(self, self._stream_checks("encode_sessions", capacity, device), capacity)

    def decode_sessions(self, capacity: int, device=None) -> "EncodecDecodeSessions":
        """The decode side of `encode_sessions`: `push(slots, toks)` returns every listed session's samples."""
        return EncodecDecodeSessions(self, self._stream_checks("decode_sessions", capacity, device), capacity)

    # ---- measurement hook used by bench.py ------------------------------------------------------
    def profile_kernels(self, fn):
        """Run fn() with per-kernel HIP-event timing armed; returns [(name, launches, ms, flops, bytes)]."""
        nat = self._native_for(torch.empty(0, device=torch.device("cuda", torch.cuda.current_device())))
        _native.check(nat.lib.ac_profile_begin(nat.h), nat.h, "ac_profile_begin")
        try:
            fn()
        finally:
            buf = (_native.AcKernelStat * 256)()
            n = nat.lib.ac_profile_end(nat.h, buf, 256)
        _native.check(n, nat.h, "ac_profile_end")
        return [(buf[i].name.decode(), buf[i].launches, buf[i].total_ms, buf[i].flops, buf[i].bytes) for i in range(n)]


class _EncodecStream:
    """What the two directions share: the device-side state block, the grow-only workspace and the warm-up rule.

    EnCodec pads every causal conv by REFLECTION, so the first rows of a clip see a mirror image of the rows that follow them.  A
    stream can reproduce that only once those rows are there: it holds back its first `WARMUP_FRAMES` = max(kernel_size,
    last_kernel_size) frames (7 frames = 93 ms at 75 frames/s) and runs them as one push.  With fewer the reference itself switches
    to its small-input padding rule and the one-shot result differs (tests/test_encodec_stream_oracle.py): the hold is the
    reference's padding, not a choice of this library."""

    def __init__(self, codec: Encodec, nat: _Native, batch_size: int, kind: str, resample: bool = False):
        self.codec = codec
        self._nat = nat
        self.batch_size = batch_size
        self.num_codebooks = codec._num_quantizers()
        self.hop = codec.config.hop_length
        self.WARMUP_FRAMES = max(codec.config.kernel_size, codec.config.last_kernel_size)
        self.device = nat.device
        L = nat.lib
        self._fns = {
            "encode": (L.ac_encodec_stream_state_bytes, L.ac_encodec_stream_reset, L.ac_encodec_stream_workspace_bytes, L.ac_encodec_stream_encode),
            "decode": (L.ac_encodec_stream_decode_state_bytes, L.ac_encodec_stream_decode_reset, L.ac_encodec_stream_decode_workspace_bytes,
                       L.ac_encodec_stream_decode),
        }[kind]
        self._kind = kind
        nbytes = self._fns[0](nat.h, batch_size)
        if nbytes == 0:
            raise _native.NativeError(f"ac_encodec_stream_{'decode_' if kind == 'decode' else ''}state_bytes returned 0")
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self._ws = None
        self.frames = 0          # frames run so far (the same for every slot)
        # resample=True at another rate than the codec's: the boundary's resampler, in front of the encoder or behind the decoder
        self._rs = None
        self._finished = False
        rate, own = int(codec.sample_rate), int(codec.config.sampling_rate)
        if resample and rate != own:
            self._rs = ResampleStream(rate, own, batch_size, self.device) if kind == "encode" else ResampleStream(own, rate, batch_size, self.device)

    def _open(self, what: str) -> None:
        if self._finished:
            raise ValueError(f"{what} after finish: the stream is closed (call reset() first)")

    def _reset_native(self, streams) -> None:
        if streams is not None:
            raise ValueError(
                "EnCodec streams reset together: a slot restarted alone would sit in its warm-up hold while the others run "
                "(`streams` must be None)"
            )
        nat = self._nat
        with torch.cuda.device(self.device):
            _native.check(self._fns[1](nat.h, _ptr(self._state), self._state.numel(), self.batch_size, None, _stream()), nat.h,
                          f"ac_encodec_stream_{self._kind}_reset")
        self.frames = 0
        self._finished = False
        if self._rs is not None:
            self._rs.reset()

    def _run(self, src: torch.Tensor, n: int, dst: torch.Tensor) -> None:
        nat = self._nat
        with torch.cuda.device(self.device):
            need = self._fns[2](nat.h, self.batch_size, n)
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
            _native.check(self._fns[3](nat.h, _ptr(self._state), self._state.numel(), _ptr(src), self.batch_size, n, self.num_codebooks, _ptr(dst),
                                       _ptr(self._ws), self._ws.numel(), _stream()), nat.h, f"ac_encodec_stream_{self._kind}")
        self.frames += n


class EncodecEncodeStream(_EncodecStream):
    """Streaming EnCodec encode of `batch_size` streams (Encodec.encode_stream).  `push(sig)` takes [B, L] fp32 samples on the
    codec's device, any L >= 0, and returns the int64 tokens [B, n, K] of the frames it releases (n may be 0).  Samples that do not
    fill a frame wait here (`pending` samples).  A fresh stream releases nothing until `WARMUP_FRAMES` whole frames are in (the
    reference's reflect padding: 93 ms); the push that crosses that mark returns all frames completed so far, and from then on every
    frame comes out in the push that completes it.  The tokens of a stream are those `sig_to_toks` gives on its whole signal (up to
    near-ties: scales are taken per push), however it was split into pushes and whatever the other streams carry.  The stream state
    and the workspace are device tensors owned by this object.

    With `resample=True` on a codec whose `sample_rate` is not the model's, `push` takes samples at `sample_rate`; they pass a
    `ResampleStream` (0.5 ms of added latency for 16 -> 24 kHz) and the frame and warm-up rules above then count resampled samples.
    `finish()` flushes the resampler's tail into the encoder and returns the tokens of any frame that completes; a trailing partial
    frame stays `pending`.  After `finish` only `reset` is accepted."""

    def __init__(self, codec: Encodec, nat: _Native, batch_size: int, resample: bool = False):
        super().__init__(codec, nat, batch_size, "encode", resample)
        self._pending = torch.empty(batch_size, 0, dtype=torch.float32, device=self.device)
        self.reset()

    @property
    def pending(self) -> int:
        return int(self._pending.shape[1])

    @torch.no_grad()
    def reset(self, streams=None) -> None:
        """Start all streams afresh, dropping what is pending (held warm-up frames included).  `streams` must be None."""
        self._reset_native(streams)
        self._pending = self._pending[:, :0]

    @torch.no_grad()
    def push(self, sig: torch.Tensor) -> torch.Tensor:
        B = self.batch_size
        if not isinstance(sig, torch.Tensor) or sig.dim() != 2 or sig.shape[0] != B:
            raise ValueError(f"push expects a [{B}, L] tensor, got {tuple(sig.shape) if isinstance(sig, torch.Tensor) else type(sig)}")
        if sig.dtype != torch.float32:
            raise ValueError(f"push expects float32 samples, got {sig.dtype}")
        if sig.device != self.device:
            raise ValueError(f"push expects samples on {self.device}, got {sig.device}")
        self._open("push")
        return self._take(self._resampled(sig, False) if self._rs is not None else sig)

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """Close the streams: the resampler's tail goes through the encoder; returns the tokens [B, n, K] of the frames it completes."""
        self._open("finish")
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
        n = (self.pending + sig.shape[1]) // hop
        if n == 0 or (self.frames == 0 and n < self.WARMUP_FRAMES):
            self._pending = torch.cat([self._pending, sig], 1) if sig.shape[1] else self._pending
            return torch.empty(B, 0, K, dtype=torch.int64, device=self.device)
        whole = torch.cat([self._pending, sig], 1) if self.pending else sig
        chunk = whole[:, : n * hop].contiguous()
        toks = torch.empty(B, n, K, dtype=torch.int64, device=self.device)
        self._run(chunk, n, toks)
        self._pending = whole[:, n * hop:].clone()
        return toks


class EncodecDecodeStream(_EncodecStream):
    """Streaming EnCodec decode of `batch_size` streams (Encodec.decode_stream).  `push(toks)` takes [B, F, K] int64 tokens on the
    codec's device, K = the codec's stage count, any F >= 0, and returns [B, n * hop] fp32 samples.  A fresh stream holds its first
    tokens back (`pending_frames`) until `WARMUP_FRAMES` frames are in (the reference's reflect padding), returns the samples of all
    of them with the push that crosses that mark, and F * hop samples per push from then on.  The samples of a stream are those
    `toks_to_sig` gives on its whole token sequence (up to rounding), whatever the other streams carry.  The stream state and the
    workspace are device tensors owned by this object.

    With `resample=True` on a codec whose `sample_rate` is not the model's, the samples pass a `ResampleStream` to `sample_rate` on
    their way out: a push returns what the resampler has completed (the count varies), `finish()` its tail, and everything together
    has the length `toks_to_sig` returns.  After `finish` only `reset` is accepted."""

    def __init__(self, codec: Encodec, nat: _Native, batch_size: int, resample: bool = False):
        super().__init__(codec, nat, batch_size, "decode", resample)
        self._held = torch.empty(batch_size, 0, self.num_codebooks, dtype=torch.int64, device=self.device)
        self.reset()

    @property
    def pending_frames(self) -> int:
        return int(self._held.shape[1])

    @torch.no_grad()
    def reset(self, streams=None) -> None:
        """Start all streams afresh, dropping the held warm-up frames.  `streams` must be None."""
        self._reset_native(streams)
        self._held = self._held[:, :0]

    @torch.no_grad()
    def push(self, toks: torch.Tensor) -> torch.Tensor:
        B, K = self.batch_size, self.num_codebooks
        if not isinstance(toks, torch.Tensor) or toks.dim() != 3 or toks.shape[0] != B or toks.shape[2] != K:
            raise ValueError(f"push expects a [{B}, F, {K}] tensor, got {tuple(toks.shape) if isinstance(toks, torch.Tensor) else type(toks)}")
        if toks.dtype != torch.int64:
            raise ValueError(f"push expects int64 tokens, got {toks.dtype}")
        if toks.device != self.device:
            raise ValueError(f"push expects tokens on {self.device}, got {toks.device}")
        self._open("push")
        sig = self._decode(toks)
        return self._rs.push(sig) if self._rs is not None else sig

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """Close the streams: the resampler's tail [B, m] (nothing without one).  Held warm-up frames are not decoded."""
        self._open("finish")
        self._finished = True
        if self._rs is not None:
            return self._rs.finish()
        return torch.empty(self.batch_size, 0, dtype=torch.float32, device=self.device)

    def _decode(self, toks: torch.Tensor) -> torch.Tensor:
        B, hop, K = self.batch_size, self.hop, self.num_codebooks
        n = self.pending_frames + toks.shape[1]
        if n == 0 or (self.frames == 0 and n < self.WARMUP_FRAMES):
            self._held = torch.cat([self._held, toks], 1) if toks.shape[1] else self._held
            return torch.empty(B, 0, dtype=torch.float32, device=self.device)
        chunk = (torch.cat([self._held, toks], 1) if self.pending_frames else toks).contiguous()
        sig = torch.empty(B, n * hop, dtype=torch.float32, device=self.device)
        self._run(chunk, n, sig)
        self._held = self._held[:, :0]
        return sig


class _EncodecSessions:
    """A pool of independent sessions on one EnCodec stream state (include/audiocodecs_amd.h ac_encodec_stream_*_slots).

    The state holds `capacity` slots.  `open` hands out the lowest free one and restarts it alone; `push(slots, x)` runs any subset,
    row i of `x` belonging to `slots[i]`.  A slot follows the rule a whole lockstep stream follows (`_EncodecStream`): partial frames
    wait, a fresh slot holds until `WARMUP_FRAMES` whole frames are in and releases them in one go.  The rows of a push that run the
    same number of frames share one native call, the groups going out in ascending F (sessions.plan_push); a slot's bits are those of
    a lone stream fed the same pieces, whichever slot it sits in and whatever the others do."""

    _unit = 1          # units per frame in what a slot holds back: samples on the encode side, token frames on the decode side

    def __init__(self, codec: Encodec, nat: _Native, capacity: int, kind: str):
        self.codec = codec
        self._nat = nat
        self.capacity = capacity
        self.num_codebooks = codec._num_quantizers()
        self.hop = codec.config.hop_length
        self.WARMUP_FRAMES = max(codec.config.kernel_size, codec.config.last_kernel_size)
        self.device = nat.device
        L = nat.lib
        self._fns = {
            "encode": (L.ac_encodec_stream_state_bytes, L.ac_encodec_stream_reset, L.ac_encodec_stream_workspace_bytes,
                       L.ac_encodec_stream_encode_slots, L.ac_encodec_stream_reset_slots),
            "decode": (L.ac_encodec_stream_decode_state_bytes, L.ac_encodec_stream_decode_reset, L.ac_encodec_stream_decode_workspace_bytes,
                       L.ac_encodec_stream_decode_slots, L.ac_encodec_stream_decode_reset_slots),
        }[kind]
        self._kind = kind
        nbytes = self._fns[0](nat.h, capacity)
        if nbytes == 0:
            raise _native.NativeError(f"ac_encodec_stream_{'decode_' if kind == 'decode' else ''}state_bytes returned 0")
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self._ws = None
        self._is_open = [False] * capacity
        self._ran = [0] * capacity              # frames run since the slot was opened
        self._held = [self._empty()] * capacity  # what waits per slot: [m] samples / [m, K] tokens
        with torch.cuda.device(self.device):    # the one whole reset: the header, and the handle's record of the address
            _native.check(self._fns[1](nat.h, _ptr(self._state), self._state.numel(), capacity, None, _stream()), nat.h,
                          f"ac_encodec_stream_{kind}_reset")

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
        """Units of `slot` that have not run: samples on the encode side, token frames on the decode side."""
        return int(self._held[self._slot(slot)].shape[0])

    def frames(self, slot: int) -> int:
        """Frames `slot` has run since it was opened."""
        return self._ran[self._slot(slot)]

    def _slot_lists(self, slots):
        host = (C.c_int * len(slots))(*slots)
        return host, torch.tensor(list(slots), dtype=torch.int32, device=self.device)

    @torch.no_grad()
    def open(self) -> int:
        """Take the lowest free slot and restart it alone (the others keep running); ValueError when the pool is full."""
        free = [s for s in range(self.capacity) if not self._is_open[s]]
        if not free:
            raise ValueError(f"the pool is full: all {self.capacity} slots are open")
        slot = free[0]
        nat = self._nat
        with torch.cuda.device(self.device):
            host, dev = self._slot_lists([slot])
            _native.check(self._fns[4](nat.h, _ptr(self._state), self._state.numel(), self.capacity, host, _ptr(dev), 1, _stream()), nat.h,
                          f"ac_encodec_stream_{self._kind}_reset_slots")
        self._is_open[slot] = True
        self._ran[slot] = 0
        self._held[slot] = self._empty()
        return slot

    def close(self, slot: int) -> None:
        """Free `slot`, dropping what it holds (held warm-up frames included)."""
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
            host, dev = self._slot_lists(slots)
            _native.check(self._fns[3](nat.h, _ptr(self._state), self._state.numel(), self.capacity, host, _ptr(dev), n, _ptr(src), F,
                                       self.num_codebooks, _ptr(dst), _ptr(self._ws), self._ws.numel(), _stream()), nat.h,
                          f"ac_encodec_stream_{self._kind}_slots")
        for s in slots:
            self._ran[s] += F

    @torch.no_grad()
    def push(self, slots, x: torch.Tensor):
        """Feed row i of `x` to `slots[i]` (n distinct open slots); returns n tensors, what each slot releases (possibly nothing)."""
        slots = self._check_push(slots, x)
        unit = self._unit
        whole = [torch.cat([self._held[s], x[i]], 0) if self._held[s].shape[0] else x[i] for i, s in enumerate(slots)]
        plan = plan_push([int(self._held[s].shape[0]) for s in slots], [self._ran[s] for s in slots], [int(x.shape[1])] * len(slots),
                         unit, self.WARMUP_FRAMES)
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


class EncodecEncodeSessions(_EncodecSessions):
    """A pool of encode sessions (Encodec.encode_sessions).  `push(slots, sig)`: `sig` is [n, L] fp32 on the codec's device, any
    L >= 0; returns n int64 tensors [f_i, K], the tokens of the frames each slot releases."""

    def __init__(self, codec: Encodec, nat: _Native, capacity: int):
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


class EncodecDecodeSessions(_EncodecSessions):
    """A pool of decode sessions (Encodec.decode_sessions).  `push(slots, toks)`: `toks` is [n, F, K] int64 on the codec's device,
    K = the codec's stage count, any F >= 0; returns n fp32 tensors [f_i * hop], the samples of the frames each slot releases."""

    def __init__(self, codec: Encodec, nat: _Native, capacity: int):
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
