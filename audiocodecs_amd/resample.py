"""Sample-rate conversion at the Codec boundary.

The reference calls ``torchaudio.functional.resample(sig, orig, new)`` with torchaudio's defaults
(/root/reference/audiocodecs/codec.py:59-63,95-99): ``sinc_interp_hann``, lowpass_filter_width 6,
rolloff 0.99.  torchaudio is not on disk here (pinned 2.4.0 in downstream/environment.yml:244), so
the filter bank below restates its published algorithm -- **parity with
torchaudio is unpinned**; tests check it against an fp64 restatement and against the analytic
response on band-limited tones.  Equal rates return the input unchanged, as torchaudio does.
The FIR itself runs in the HIP library (``ac_resample``); there is no CPU fallback.

``ResampleStream`` is the same conversion push by push (``ac_resample_stream_*``): it carries its filter
history and its phase on the device, and the concatenation of what it returns is bit for bit what ``resample`` gives on the whole
signal.  The codec streams use it for callers at another rate than the codec's (``encode_stream(..., resample=True)``).

``ResampleSlots`` is the same state served slot by slot (``ac_resample_stream_*_slots``): every slot stands at
its own phase, restarts alone and closes alone, and its bits are those of a lone ``ResampleStream``.  The session pools use it
(``encode_sessions(..., resample=True)``).
"""

from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Tuple

import torch

__all__ = ["resample", "sinc_kernel", "ResampleStream", "ResampleSlots", "stream_out_len"]

_LOWPASS_FILTER_WIDTH = 6
_ROLLOFF = 0.99


def sinc_kernel(orig_freq: int, new_freq: int, dtype=torch.float32) -> Tuple[torch.Tensor, int, int, int]:
    """Hann-windowed sinc filter bank [n, taps] for orig -> new (after gcd reduction) and (n, o, width).
    Computed in `dtype` like torchaudio computes it in the waveform's dtype."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base_freq = min(o, n) * _ROLLOFF
    width = math.ceil(_LOWPASS_FILTER_WIDTH * o / base_freq)
    idx = torch.arange(-width, width + o, dtype=dtype)[None] / o            # [1, taps]
    t = torch.arange(0, -n, -1, dtype=dtype)[:, None] / n + idx             # phase i: -i/n + idx
    t = (t * base_freq).clamp_(-_LOWPASS_FILTER_WIDTH, _LOWPASS_FILTER_WIDTH)
    window = torch.cos(t * math.pi / _LOWPASS_FILTER_WIDTH / 2) ** 2
    t = t * math.pi
    scale = base_freq / o
    kernels = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * scale
    return kernels.contiguous(), n, o, width


_BANKS: Dict[tuple, tuple] = {}


def resample(sig: torch.Tensor, orig_freq, new_freq) -> torch.Tensor:
    """sig [B, L] -> [B, ceil(new/orig * L)] on the GPU (identity when the rates are equal)."""
    if int(orig_freq) == int(new_freq):
        return sig
    from . import _native

    if sig.shape[0] == 0:   # an empty shard: the output shape only (the library is not called)
        g = math.gcd(int(orig_freq), int(new_freq))
        return torch.empty(0, int(math.ceil((int(new_freq) // g) * sig.shape[1] / (int(orig_freq) // g))), dtype=torch.float32, device=sig.device)
    if not sig.is_cuda:
        raise _native.NativeError("audiocodecs_amd.resample runs on MI355X only: move the signal to a cuda device")
    key = (int(orig_freq), int(new_freq), sig.device.index)
    if key not in _BANKS:
        k, n, o, width = sinc_kernel(orig_freq, new_freq)
        _BANKS[key] = (k.to(sig.device), n, o, width)
    kern, n, o, width = _BANKS[key]
    x = sig.to(torch.float32).contiguous()
    B, L = x.shape
    L_out = int(math.ceil(n * L / o))
    y = torch.empty(B, L_out, dtype=torch.float32, device=sig.device)
    with torch.cuda.device(sig.device):
        rc = _native.lib().ac_resample(
            C.c_void_p(x.data_ptr()), B, L, C.c_void_p(kern.data_ptr()), n, o, kern.shape[1], width,
            C.c_void_p(y.data_ptr()), L_out, C.c_void_p(torch.cuda.current_stream().cuda_stream),
        )
    _native.check(rc, None, "ac_resample")
    return y


def stream_out_len(consumed: int, L: int, n: int, o: int, width: int, finish: bool = False) -> int:
    """Samples per stream that a push of L samples emits on a stream that has consumed `consumed` (with `finish`: that push as the
    closing one).  Pure host arithmetic in the library (``ac_resample_stream_out_len``); needs no GPU."""
    from . import _native

    m = _native.lib().ac_resample_stream_out_len(int(consumed), int(L), int(n), int(o), int(width), int(bool(finish)))
    if m < 0:
        raise ValueError(f"stream_out_len: bad arguments (consumed={consumed}, L={L}, n={n}, o={o}, width={width})")
    return int(m)


def _positive_int(name, v) -> int:
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"`{name}` ({v!r}) must be a positive int")
    return v


class ResampleStream:
    """Streaming sample-rate conversion of `batch_size` streams that share one phase: `push(sig)` takes [B, L] fp32 samples at
    `orig_freq`, any L >= 0, and returns the [B, m] samples at `new_freq` that no later input can change -- m varies from push to push
    and may be 0; `finish()` takes all later input as silence and returns the rest, after which only `reset()` is accepted.  The
    concatenated output is bit for bit `resample(whole signal)`, however the signal was split.  Output lags input by
    `latency_samples` = width + o - 1 input samples (0.5 ms for 16 <-> 24 kHz).  Equal rates pass the input through.  The state is a
    device tensor owned by this object; every call runs on the current stream and neither allocates in the library nor synchronises."""

    def __init__(self, orig_freq: int, new_freq: int, batch_size: int, device=None):
        self.orig_freq, self.new_freq = _positive_int("orig_freq", orig_freq), _positive_int("new_freq", new_freq)
        self.batch_size = _positive_int("batch_size", batch_size)
        self.identity = self.orig_freq == self.new_freq
        self.consumed = 0        # input samples taken since the reset (the same for every slot)
        self.emitted = 0         # output samples returned since the reset
        self._finished = False
        if self.identity:
            self.device = None if device is None else torch.device(device)
            self.n = self.o = 1
            self.width = self.taps = 0
            return
        from . import _native

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise _native.NativeError("audiocodecs_amd.ResampleStream runs on MI355X only: give it a cuda device")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        kern, self.n, self.o, self.width = sinc_kernel(self.orig_freq, self.new_freq)
        self.taps = int(kern.shape[1])
        self._lib = _native.lib()
        nbytes = self._lib.ac_resample_stream_state_bytes(self.batch_size, self.taps)
        if nbytes == 0:
            raise _native.NativeError(f"ac_resample_stream_state_bytes returned 0 (B={self.batch_size}, taps={self.taps})")
        self._kern = kern.to(self.device)
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self.reset()

    @property
    def latency_samples(self) -> int:
        """Input samples that must follow a sample before the outputs it bears on are complete."""
        return 0 if self.identity else self.width + self.o - 1

    def out_len(self, L: int, finish: bool = False) -> int:
        """Samples per stream the next `push` of L samples (`finish=True`: that push as the closing one) returns."""
        if self.identity:
            return int(L)
        return stream_out_len(self.consumed, L, self.n, self.o, self.width, finish)

    @torch.no_grad()
    def reset(self) -> None:
        """Start all streams afresh."""
        self.consumed = self.emitted = 0
        self._finished = False
        if self.identity:
            return
        from . import _native

        with torch.cuda.device(self.device):
            rc = self._lib.ac_resample_stream_reset(C.c_void_p(self._state.data_ptr()), self._state.numel(), self.batch_size, self.n, self.o,
                                                    self.taps, self.width, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, None, "ac_resample_stream_reset")

    def _run(self, x, L: int, finish: bool, out):
        from . import _native

        B = self.batch_size
        m = self.out_len(L, finish)
        if out is None:
            out = torch.empty(B, m, dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dim() != 2 or out.shape != (B, m) or out.dtype != torch.float32 or out.device != self.device
              or (m and out.stride(1) != 1) or (m and B > 1 and out.stride(0) < m)):
            raise ValueError(f"`out` must be a [{B}, {m}] float32 tensor on {self.device} with unit stride along its rows")
        if L or finish:
            if L and (x.stride(1) != 1 or (B > 1 and x.stride(0) < L)):
                x = x.contiguous()
            with torch.cuda.device(self.device):
                rc = self._lib.ac_resample_stream_push(
                    C.c_void_p(self._state.data_ptr()), self._state.numel(), C.c_void_p(x.data_ptr() if L else 0), max(x.stride(0), L) if L else 0, B, L,
                    self.consumed, C.c_void_p(self._kern.data_ptr()), self.n, self.o, self.taps, self.width,
                    C.c_void_p(out.data_ptr() if m else 0), max(out.stride(0), m), m, int(finish), C.c_void_p(torch.cuda.current_stream().cuda_stream),
                )
            _native.check(rc, None, "ac_resample_stream_push")
        self.consumed += L
        self.emitted += m
        self._finished = finish
        return out

    @torch.no_grad()
    def push(self, sig: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
        """sig [B, L] fp32 -> [B, m].  `out`: where to write them -- a [B, out_len(L)] fp32 tensor whose rows may be further apart than
        they are long (a column slice of a larger buffer: the samples land straight behind those the caller already holds)."""
        B = self.batch_size
        if not isinstance(sig, torch.Tensor) or sig.dim() != 2 or sig.shape[0] != B:
            raise ValueError(f"push expects a [{B}, L] tensor, got {tuple(sig.shape) if isinstance(sig, torch.Tensor) else type(sig)}")
        if sig.dtype != torch.float32:
            raise ValueError(f"push expects float32 samples, got {sig.dtype}")
        if self._finished:
            raise ValueError("push after finish: the stream is closed (call reset() first)")
        if self.identity:
            self.consumed += sig.shape[1]
            self.emitted += sig.shape[1]
            if out is not None:
                out.copy_(sig)
                return out
            return sig
        if sig.device != self.device:
            raise ValueError(f"push expects samples on {self.device}, got {sig.device}")
        return self._run(sig, int(sig.shape[1]), False, out)

    @torch.no_grad()
    def finish(self, out: torch.Tensor = None) -> torch.Tensor:
        """Close the streams: what `resample` on the whole signal still has beyond the samples returned so far, [B, m]."""
        if self._finished:
            raise ValueError("finish after finish: the stream is closed (call reset() first)")
        if self.identity:
            self._finished = True
            return torch.empty(self.batch_size, 0, dtype=torch.float32, device=self.device) if out is None else out
        return self._run(None, 0, True, out)


class ResampleSlots:
    """Streaming sample-rate conversion of up to `capacity` independent streams ("slots") on one state, each at its own phase.
    `push(slots, sig)` takes [n, L] fp32 samples at `orig_freq`, row i for `slots[i]`, and returns n tensors [m_i]: the samples at
    `new_freq` of that slot that no later input can change (m_i differs from row to row and may be 0).  `push(..., finish=True)`
    closes the listed slots: it takes all later input as silence and returns the rest; a closed slot accepts only `restart`.
    `restart(slots)` starts the listed slots afresh while the others keep what they hold.  Per slot the concatenated output is bit
    for bit `resample(its whole signal)`, whichever slot it sits in, whatever the other rows carry and however many pushes it sits
    out.  Equal rates pass the input through.  `consumed[s]` / `emitted[s]` count slot s's samples since its restart.  The state is a
    device tensor owned by this object; a push is one host-to-device copy (slots and counts together) and two launches on the
    current stream, and neither allocates in the library nor synchronises."""

    def __init__(self, orig_freq: int, new_freq: int, capacity: int, device=None):
        self.orig_freq, self.new_freq = _positive_int("orig_freq", orig_freq), _positive_int("new_freq", new_freq)
        self.capacity = _positive_int("capacity", capacity)
        self.identity = self.orig_freq == self.new_freq
        self.consumed = [0] * capacity       # input samples taken per slot since its restart
        self.emitted = [0] * capacity        # output samples returned per slot since its restart
        self._finished = [False] * capacity
        if self.identity:
            self.device = None if device is None else torch.device(device)
            self.n = self.o = 1
            self.width = self.taps = 0
            return
        kern, self.n, self.o, self.width = sinc_kernel(self.orig_freq, self.new_freq)
        self.taps = int(kern.shape[1])
        self._attach(kern, device)

    @property
    def latency_samples(self) -> int:
        """Input samples that must follow a sample before the outputs it bears on are complete."""
        return 0 if self.identity else self.width + self.o - 1

    # -- the device side: everything that touches the library's state (a subclass on CPU tensors replaces these three) ---------------------
    def _attach(self, kern: torch.Tensor, device) -> None:
        """Allocate the state of `capacity` slots and reset it whole (the one call that writes its header)."""
        from . import _native

        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise _native.NativeError("audiocodecs_amd.ResampleSlots runs on MI355X only: give it a cuda device")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self._lib = _native.lib()
        nbytes = self._lib.ac_resample_stream_state_bytes(self.capacity, self.taps)
        if nbytes == 0:
            raise _native.NativeError(f"ac_resample_stream_state_bytes returned 0 (B={self.capacity}, taps={self.taps})")
        self._kern = kern.to(self.device)
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        with torch.cuda.device(self.device):
            rc = self._lib.ac_resample_stream_reset(C.c_void_p(self._state.data_ptr()), self._state.numel(), self.capacity, self.n, self.o,
                                                    self.taps, self.width, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, None, "ac_resample_stream_reset")

    def _restart_rows(self, slots) -> None:
        from . import _native

        n = len(slots)
        with torch.cuda.device(self.device):
            dev = torch.tensor(slots, dtype=torch.int32, device=self.device)
            rc = self._lib.ac_resample_stream_reset_slots(
                C.c_void_p(self._state.data_ptr()), self._state.numel(), self.capacity, self.n, self.o, self.taps, self.width,
                (C.c_int * n)(*slots), C.c_void_p(dev.data_ptr()), n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, None, "ac_resample_stream_reset_slots")

    def _push_rows(self, slots, counts, x, L: int, m: int, finish: bool) -> torch.Tensor:
        """One native push: row i of x [n, L] to slots[i], which stands at counts[i]; returns y [n, m], m the longest row's output."""
        from . import _native

        n = len(slots)
        y = torch.empty(n, m, dtype=torch.float32, device=self.device)
        if L and (x.stride(1) != 1 or (n > 1 and x.stride(0) < L)):
            x = x.contiguous()
        desc = torch.empty(n + (n + 1) // 2, dtype=torch.int64)     # counts [n] int64, then slots [n] int32: one copy to the device
        desc[:n] = torch.tensor(counts, dtype=torch.int64)
        desc[n:].view(torch.int32)[:n] = torch.tensor(slots, dtype=torch.int32)
        with torch.cuda.device(self.device):
            dev = desc.to(self.device)
            rc = self._lib.ac_resample_stream_push_slots(
                C.c_void_p(self._state.data_ptr()), self._state.numel(), self.capacity, (C.c_int * n)(*slots), (C.c_longlong * n)(*counts),
                C.c_void_p(dev.data_ptr() + 8 * n), C.c_void_p(dev.data_ptr()), n, C.c_void_p(x.data_ptr() if L else 0),
                max(x.stride(0), L) if L else 0, L, C.c_void_p(self._kern.data_ptr()), self.n, self.o, self.taps, self.width,
                C.c_void_p(y.data_ptr() if m else 0), m, m, int(finish), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.check(rc, None, "ac_resample_stream_push_slots")
        return y

    # -- the host side -----------------------------------------------------------------------------------------------------------------
    def _slots(self, what: str, slots):
        try:
            slots = list(slots)
        except TypeError:
            raise ValueError(f"{what} expects a sequence of slots, got {type(slots)}")
        if any(isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < self.capacity for s in slots):
            raise ValueError(f"{what}: `slots` ({slots!r}) must list slots in [0, {self.capacity})")
        if len(set(slots)) != len(slots):
            raise ValueError(f"{what}: a slot is listed twice in {slots}")
        return slots

    def out_len(self, slot: int, L: int, finish: bool = False) -> int:
        """Samples the next `push` of L samples (`finish=True`: that push as the closing one) returns for `slot`."""
        slot, = self._slots("out_len", [slot])
        if self.identity:
            return int(L)
        return stream_out_len(self.consumed[slot], L, self.n, self.o, self.width, finish)

    @torch.no_grad()
    def restart(self, slots) -> None:
        """Start the listed slots afresh; the others keep what they hold."""
        slots = self._slots("restart", slots)
        if slots and not self.identity:
            self._restart_rows(slots)
        for s in slots:
            self.consumed[s] = self.emitted[s] = 0
            self._finished[s] = False

    @torch.no_grad()
    def push(self, slots, sig: torch.Tensor, finish: bool = False):
        """sig [n, L] fp32, row i for slots[i] -> n tensors [m_i].  `finish=True`: the push closes the listed slots."""
        slots = self._slots("push", slots)
        n = len(slots)
        if not isinstance(sig, torch.Tensor) or sig.dim() != 2 or sig.shape[0] != n:
            raise ValueError(f"push expects a [{n}, L] tensor, got {tuple(sig.shape) if isinstance(sig, torch.Tensor) else type(sig)}")
        if sig.dtype != torch.float32:
            raise ValueError(f"push expects float32 samples, got {sig.dtype}")
        for s in slots:
            if self._finished[s]:
                raise ValueError(f"push after finish: slot {s} is closed (call restart([{s}]) first)")
        if not self.identity and sig.device != self.device:
            raise ValueError(f"push expects samples on {self.device}, got {sig.device}")
        L = int(sig.shape[1])
        ms = [self.out_len(s, L, finish) for s in slots]
        if self.identity:
            out = [sig[i] for i in range(n)]
        elif n and (L or finish):
            y = self._push_rows(slots, [self.consumed[s] for s in slots], sig, L, max(ms), bool(finish))
            out = [y[i, :m] for i, m in enumerate(ms)]
        else:
            out = [torch.empty(0, dtype=torch.float32, device=self.device) for _ in slots]
        for s, m in zip(slots, ms):
            self.consumed[s] += L
            self.emitted[s] += m
            self._finished[s] = bool(finish)
        return out
