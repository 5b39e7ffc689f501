"""The host side every streaming surface shares (Encodec / Mimi `encode_stream`, `decode_stream`, and through sessions.py the session
pools): one lockstep stream, written once for both directions and both codecs.

What differs between codecs and directions sits in one small backend object per (codec, direction): `StreamBackend` makes every native
call (include/audiocodecs_amd.h ac_*_stream_*) and carries the facts the host logic needs -- the warm-up hold, the transformer
positions a frame takes, whether single slots of a lockstep stream may restart.  The classes here touch tensors on `self.device` only;
device contexts, streams, ctypes arrays and the device slot list belong to the backend, so the hold / release logic runs on CPU tensors
with a toy backend (tests/test_stream_host.py)."""

from __future__ import annotations

import ctypes as C

import torch

from . import _native
from ._native import _ptr, _stream
from .resample import ResampleStream

__all__ = ["StreamBackend", "StreamHost", "LockstepStream", "stream_checks"]


class StreamBackend:
    """Every native call of one codec's streams in one direction (`kind`: "encode" / "decode"), on the handle `nat`.  `prefix` names the
    entry points ("ac_mimi_stream": ac_mimi_stream_reset, ac_mimi_stream_decode_slots, ...).

    `warmup`: whole frames a fresh stream must bring to its first run (1: no hold).  `stride`: transformer positions per frame, counted
    against the owner's `MAX_POSITIONS`.  `reset_together`: why single slots of a lockstep stream cannot restart, or None when they can."""

    reset_together = None

    def __init__(self, nat, prefix: str, kind: str, hop: int, warmup: int = 1, stride: int = 1):
        self._nat = nat
        self.device = nat.device
        self.kind, self.hop, self.warmup, self.stride = kind, hop, warmup, stride
        d = "decode_" if kind == "decode" else ""
        self._fn = {op: getattr(nat.lib, name) for op, name in (
            ("state_bytes", f"{prefix}_{d}state_bytes"), ("reset", f"{prefix}_{d}reset"), ("workspace_bytes", f"{prefix}_{d}workspace_bytes"),
            ("push", f"{prefix}_{kind}"), ("push_slots", f"{prefix}_{kind}_slots"))}
        self._who = {"state_bytes": f"{prefix}_{d}state_bytes", "reset": f"{prefix}_{d}reset", "push": f"{prefix}_{kind}"}

    def state_bytes(self, n: int) -> int:
        nbytes = self._fn["state_bytes"](self._nat.h, n)
        if nbytes == 0:
            raise _native.NativeError(f"{self._who['state_bytes']} returned 0")
        return nbytes

    def reset(self, state: torch.Tensor, n: int, mask=None) -> None:
        """Write the header and start all `n` streams afresh, or (device `mask`, uint8 [n]) only the marked ones."""
        nat = self._nat
        with torch.cuda.device(self.device):
            _native.check(self._fn["reset"](nat.h, _ptr(state), state.numel(), n, _ptr(mask), _stream()), nat.h, self._who["reset"])

    def restart_slots(self, state: torch.Tensor, cap: int, slots) -> None:
        """Start the listed slots afresh, the others keep running: here as a masked reset."""
        mask = torch.zeros(cap, dtype=torch.uint8)
        mask[slots] = 1
        self.reset(state, cap, mask.to(self.device))

    def workspace_bytes(self, n: int, F: int) -> int:
        return self._fn["workspace_bytes"](self._nat.h, n, F)

    def run(self, state: torch.Tensor, cap: int, slots, src: torch.Tensor, F: int, K: int, dst: torch.Tensor, ws: torch.Tensor) -> None:
        """F frames for all `cap` streams of the state in order (`slots` None), or for the listed ones: row i of src / dst is slots[i]."""
        nat = self._nat
        with torch.cuda.device(self.device):
            if slots is None:
                rc = self._fn["push"](nat.h, _ptr(state), state.numel(), _ptr(src), cap, F, K, _ptr(dst), _ptr(ws), ws.numel(), _stream())
            else:
                n = len(slots)
                host = (C.c_int * n)(*slots)
                dev = torch.tensor(slots, dtype=torch.int32, device=self.device)
                rc = self._fn["push_slots"](nat.h, _ptr(state), state.numel(), cap, host, _ptr(dev), n, _ptr(src), F, K, _ptr(dst), _ptr(ws),
                                            ws.numel(), _stream())
        _native.check(rc, nat.h, self._who["push"] if slots is None else self._who["push"] + "_slots")


def stream_checks(codec, name: str, what: str, n, device, resample: bool, validate):
    """What `encode_stream` / `decode_stream` / `encode_sessions` / `decode_sessions` of the wrapper `name` refuse; returns the handle."""
    need, lacks = ("encoder", "decode") if what.startswith("encode") else ("decoder", "encode")
    pool = what.endswith("sessions")
    if codec.mode == lacks:
        raise ValueError(f"{what} needs the {need}: this {name} was built with mode=\"{lacks}\"")
    if codec.sample_rate != codec.config.sampling_rate and not resample:
        raise ValueError(
            f"{what} runs at the codec's own rate ({codec.config.sampling_rate} Hz): streaming resampling from or to "
            f"sample_rate={codec.sample_rate} is opt-in, pass resample=True"
        )
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"`{'capacity' if pool else 'batch_size'}` ({n!r}) must be a positive int")
    validate()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return codec._native_for(torch.empty(0, device=dev))


class StreamHost:
    """What a lockstep stream and a session pool own alike: the 256-byte aligned state block of `n` streams, the grow-only workspace, and
    the shapes of the two payloads -- [rows, L] fp32 samples, [rows, F, K] int64 tokens; an encoder takes the first and returns the second,
    a decoder the reverse.  Input waits in units: samples on the encode side (`hop` per frame), token frames on the decode side (1)."""

    MAX_POSITIONS = None        # transformer positions a stream may reach (codecs with position-dependent state set it)

    def __init__(self, codec, backend, n: int, num_codebooks: int):
        self.codec = codec
        self._be = backend
        self._n = n
        self.num_codebooks = num_codebooks
        self.hop = backend.hop
        self.device = backend.device
        self._encode = backend.kind == "encode"
        self._unit = self.hop if self._encode else 1
        nbytes = backend.state_bytes(n)
        self._state_buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        off = (-self._state_buf.data_ptr()) % 256
        self._state = self._state_buf[off:off + nbytes]
        self._ws = None

    def _no_input(self, *rows) -> torch.Tensor:
        """Zero units of input for `rows` rows (none: one row's own tensor)."""
        return (torch.empty(*rows, 0, dtype=torch.float32, device=self.device) if self._encode
                else torch.empty(*rows, 0, self.num_codebooks, dtype=torch.int64, device=self.device))

    def _output(self, *shape) -> torch.Tensor:
        """The result tensor of F frames: _output(rows, F), or one row's own _output(F)."""
        if self._encode:
            return torch.empty(*shape, self.num_codebooks, dtype=torch.int64, device=self.device)
        return torch.empty(*shape[:-1], shape[-1] * self.hop, dtype=torch.float32, device=self.device)

    def _check_rows(self, n: int, x, slots: bool = False) -> None:
        K, enc = self.num_codebooks, self._encode
        if not isinstance(x, torch.Tensor) or x.dim() != (2 if enc else 3) or x.shape[0] != n or (not enc and x.shape[2] != K):
            form = f"[{n}, L]" if enc else f"[{n}, F, {K}]"
            tail = f" for {n} slots" if slots else ""
            raise ValueError(f"push expects a {form} tensor{tail}, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x)}")
        if x.dtype != (torch.float32 if enc else torch.int64):
            raise ValueError(f"push expects {'float32 samples' if enc else 'int64 tokens'}, got {x.dtype}")
        if x.device != self.device:
            raise ValueError(f"push expects {'samples' if enc else 'tokens'} on {self.device}, got {x.device}")

    def _run(self, slots, src: torch.Tensor, F: int, dst: torch.Tensor) -> None:
        need = self._be.workspace_bytes(self._n if slots is None else len(slots), F)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        self._be.run(self._state, self._n, slots, src, F, self.num_codebooks, dst, self._ws)


_SHARED_PHASE = ("the slots of a resampling stream share one phase: a slot restarted alone would emit a different number of samples per "
                 "push than its neighbours (`streams` must be None)")


class LockstepStream(StreamHost):
    """`batch_size` streams that advance together: every `push` brings all of them the same amount.  What does not fill a frame waits
    (`_held`); a fresh stream holds until `warmup` whole frames are in and runs them as one push; `finish` closes the streams, after
    which only `reset` is accepted.  With `resample=True` on a codec whose `sample_rate` is not the model's, a `ResampleStream` sits at
    the boundary: in front of an encoder, behind a decoder."""

    def __init__(self, codec, backend, batch_size: int, num_codebooks: int, resample: bool = False):
        super().__init__(codec, backend, batch_size, num_codebooks)
        self.batch_size = batch_size
        self._rs = None
        rate, own = int(codec.sample_rate), int(codec.config.sampling_rate)
        if resample and rate != own:
            self._rs = ResampleStream(rate, own, batch_size, self.device) if self._encode else ResampleStream(own, rate, batch_size, self.device)
        self._finished = False
        self._held = self._no_input(batch_size)
        self._frames = [0] * batch_size       # frames run per slot since its reset
        self.reset()

    @property
    def _waiting(self) -> int:
        return int(self._held.shape[1])

    def _open(self, what: str) -> None:
        if self._finished:
            raise ValueError(f"{what} after finish: the stream is closed (call reset() first)")

    @torch.no_grad()
    def reset(self, streams=None) -> None:
        """Start all streams afresh, dropping what waits (held warm-up frames included); or, where the codec allows it, only the listed
        slots (not on a resampling stream, and not while a partial frame is pending: its samples belong to every slot)."""
        be, B = self._be, self.batch_size
        if streams is None:
            be.reset(self._state, B)
            self._held = self._held[:, :0]
            self._frames = [0] * B
            self._finished = False
            if self._rs is not None:
                self._rs.reset()
            return
        if be.reset_together:
            raise ValueError(be.reset_together)
        if self._rs is not None:
            raise ValueError(_SHARED_PHASE)
        idx = [streams] if isinstance(streams, int) else list(streams)
        if any(isinstance(i, bool) or not isinstance(i, int) or not 0 <= i < B for i in idx):
            raise ValueError(f"`streams` ({streams!r}) must list slots in [0, {B})")
        if self._waiting:
            raise ValueError(f"cannot reset single streams while {self._waiting} samples of a partial frame are pending")
        be.restart_slots(self._state, B, idx)
        for i in idx:
            self._frames[i] = 0

    @torch.no_grad()
    def push(self, x: torch.Tensor) -> torch.Tensor:
        self._check_rows(self.batch_size, x)
        self._open("push")
        if self._rs is None:
            return self._take(x)
        return self._take(self._resampled(x, False)) if self._encode else self._rs.push(self._take(x))

    @torch.no_grad()
    def finish(self) -> torch.Tensor:
        """Close the streams.  Encode: the resampler's tail goes through the encoder; returns the tokens [B, n, K] of the frames it
        completes.  Decode: the resampler's tail [B, m] (nothing without one); held warm-up frames are not decoded."""
        self._open("finish")
        if self._encode:
            out = self._take(self._resampled(None, True) if self._rs is not None else self._no_input(self.batch_size))
            self._finished = True
            return out
        self._finished = True
        return self._rs.finish() if self._rs is not None else self._output(self.batch_size, 0)

    def _resampled(self, sig, finish: bool) -> torch.Tensor:
        """The pending samples with the resampler's output for this push written straight behind them (one buffer, no second copy)."""
        rs, pend = self._rs, self._waiting
        m = rs.out_len(0 if finish else sig.shape[1], finish)
        whole = torch.empty(self.batch_size, pend + m, dtype=torch.float32, device=self.device)
        if pend:
            whole[:, :pend].copy_(self._held)
        if finish:
            rs.finish(out=whole[:, pend:])
        else:
            rs.push(sig, out=whole[:, pend:])
        self._held = self._held[:, :0]
        return whole

    def _take(self, x: torch.Tensor) -> torch.Tensor:
        """Input at the codec's rate: run the frames it completes, keep the rest waiting."""
        B, unit, be = self.batch_size, self._unit, self._be
        waiting = self._waiting
        total = waiting + x.shape[1]
        n = total // unit
        if n == 0 or (n < be.warmup and min(self._frames) == 0):
            self._held = torch.cat([self._held, x], 1) if x.shape[1] else self._held
            return self._output(B, 0)
        if self.MAX_POSITIONS is not None and be.stride * (max(self._frames) + n) > self.MAX_POSITIONS:
            raise ValueError(f"a stream would pass {self.MAX_POSITIONS} transformer positions: reset it first")
        whole = torch.cat([self._held, x], 1) if waiting else x
        out = self._output(B, n)
        if total == n * unit:                 # whole frames only (every decode push): nothing to cut off, nothing left over
            self._run(None, whole.contiguous(), n, out)
            if waiting:
                self._held = self._held[:, :0]
        else:
            self._run(None, whole[:, : n * unit].contiguous(), n, out)
            self._held = whole[:, n * unit:].clone()
        self._frames = [f + n for f in self._frames]
        return out
