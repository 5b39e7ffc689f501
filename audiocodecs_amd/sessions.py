"""The grouping rule of a session pool (Encodec.encode_sessions / decode_sessions; Mimi.encode_sessions /
decode_sessions, section 8g, with warmup = 1: Mimi pads with zeros and holds nothing back), as a pure function.

A pool serves sessions that begin and end at different times on one stream state.  Every slot follows the rule a whole lockstep
stream follows (streams.py `LockstepStream._take`, one rule for both directions): units that do not fill a frame wait, and a
slot that has run nothing yet holds until `warmup` whole frames are in and then releases them all in one go.  The native push runs
the same number of frames for every row it is given, so the rows of one `push` are grouped by the number of frames they run: one
native call per group, the groups in ascending F.  `SessionPool` is the pool itself, for every codec and both directions; like the
lockstep stream it reaches the library through a backend object only, so nothing here needs a GPU (tests/test_encodec_sessions.py,
tests/test_stream_host.py).  With `resample=True` a `ResampleSlots` sits at the boundary, one resampler slot per pool slot (DESIGN.md
section 8h); the pool calls its `restart`, `out_len` and `push` and nothing else (tests/test_resample_slots.py)."""

from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from .resample import ResampleSlots
from .streams import StreamHost

__all__ = ["plan_push", "SessionPool"]


def plan_push(pending: Sequence[int], ran: Sequence[int], incoming: Sequence[int], hop: int, warmup: int) -> List[Tuple[int, List[int]]]:
    """Group the rows of one push by the frames they run.

    Row i holds `pending[i]` units that have not run, has run `ran[i]` frames since it was opened and is brought `incoming[i]` more
    units; a frame is `hop` units (samples on the encode side; tokens frames on the decode side, hop = 1).  Returns
    [(F, rows), ...] in ascending F with ascending rows: every listed row runs exactly F frames in one native call.  A row that runs
    nothing (no whole frame, or a fresh row with fewer than `warmup` whole frames) is left out; a fresh row is never in a group with
    F < warmup, and no row is in two groups."""
    if not (len(pending) == len(ran) == len(incoming)):
        raise ValueError("plan_push: pending, ran and incoming must have one entry per row")
    if hop < 1 or warmup < 1:
        raise ValueError(f"plan_push: hop ({hop}) and warmup ({warmup}) must be positive")
    groups = {}
    for i, (p, r, m) in enumerate(zip(pending, ran, incoming)):
        if p < 0 or r < 0 or m < 0:
            raise ValueError(f"plan_push: row {i} has a negative count")
        n = (p + m) // hop
        if n == 0 or (r == 0 and n < warmup):
            continue
        groups.setdefault(n, []).append(i)
    return [(F, groups[F]) for F in sorted(groups)]


class SessionPool(StreamHost):
    """A pool of independent sessions on one stream state of `capacity` slots.

    `open` hands out the lowest free slot and restarts it alone; `push(slots, x)` runs any subset, row i of `x` belonging to
    `slots[i]`.  A slot follows the rule a whole lockstep stream follows (streams.py `LockstepStream`): partial frames wait, a fresh slot
    holds until the codec's warm-up is in and releases it in one go.  The rows of a push that run the same number of frames share one
    native call, the groups going out in ascending F (`plan_push`); a slot's bits are those of a lone stream fed the same pieces,
    whichever slot it sits in and whatever the others do.

    With `resample=True` on a codec whose `sample_rate` is not the model's, a `ResampleSlots` sits at the boundary, in front of an
    encoder and behind a decoder, every pool slot at its own phase: the rows of an encode push bring different numbers of resampled
    samples, and holding, grouping and the warm-up count those.  `finish(slot)` closes a slot's resampler; after it the slot accepts
    only `close`."""

    _resampler = ResampleSlots      # (orig_freq, new_freq, capacity, device) -> an object with restart / out_len / push

    def __init__(self, codec, backend, capacity: int, num_codebooks: int, resample: bool = False):
        super().__init__(codec, backend, capacity, num_codebooks)
        self.capacity = capacity
        self._is_open = [False] * capacity
        self._done = [False] * capacity             # finished: the slot accepts only close
        self._ran = [0] * capacity                  # frames run since the slot was opened
        self._held = [self._no_input()] * capacity   # what waits per slot: [m] samples / [m, K] tokens
        self._rs = None
        rate, own = int(codec.sample_rate), int(codec.config.sampling_rate)
        if resample and rate != own:
            self._rs = self._resampler(rate, own, capacity, self.device) if self._encode else self._resampler(own, rate, capacity, self.device)
        backend.reset(self._state, capacity)        # the one whole reset: the header, and the handle's record of the address

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

    def _unfinished(self, what: str, slot: int) -> int:
        if self._done[slot]:
            raise ValueError(f"{what} after finish: slot {slot} is closed (close() it and open a new session)")
        return slot

    def pending(self, slot: int) -> int:
        """Units of `slot` that have not run: samples on the encode side (at the codec's rate), token frames on the decode side."""
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
        self._be.restart_slots(self._state, self.capacity, [slot])
        if self._rs is not None:
            self._rs.restart([slot])
        self._is_open[slot] = True
        self._done[slot] = False
        self._ran[slot] = 0
        self._held[slot] = self._no_input()
        return slot

    def close(self, slot: int) -> None:
        """Free `slot`, dropping what it holds (held warm-up frames and the resampler's tail included)."""
        slot = self._slot(slot)
        self._is_open[slot] = False
        self._held[slot] = self._no_input()

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
        self._check_rows(len(slots), x, slots=True)
        for s in slots:
            self._unfinished("push", s)
        return slots

    def _plan(self, slots, incoming):
        """The groups of a push that brings row i `incoming[i]` units (refused before anything runs where a slot would pass its limit)."""
        plan = plan_push([int(self._held[s].shape[0]) for s in slots], [self._ran[s] for s in slots], incoming, self._unit, self._be.warmup)
        if self.MAX_POSITIONS is not None:
            for F, rows in plan:
                for i in rows:
                    if self._be.stride * (self._ran[slots[i]] + F) > self.MAX_POSITIONS:
                        raise ValueError(f"slot {slots[i]} would pass {self.MAX_POSITIONS} transformer positions: close it and open a new session")
        return plan

    def _advance(self, slots, plan, rows_in):
        """Run `plan` on the rows `rows_in` (row i: what slots[i] is brought, at the codec's rate, behind what it holds); returns what
        every row releases.  On a resampling decoder each group's samples pass the resampler, every row at its own phase."""
        unit = self._unit
        whole = [torch.cat([self._held[s], rows_in[i]], 0) if self._held[s].shape[0] else rows_in[i] for i, s in enumerate(slots)]
        resampled = self._rs is not None and not self._encode
        out = [self._output(0) for _ in slots]
        for F, rows in plan:
            src = torch.stack([whole[i][: F * unit] for i in rows], 0).contiguous()
            dst = self._output(len(rows), F)
            group = [slots[i] for i in rows]
            self._run(group, src, F, dst)
            res = self._rs.push(group, dst) if resampled else dst
            for j, i in enumerate(rows):
                self._ran[slots[i]] += F
                out[i] = res[j]
                whole[i] = whole[i][F * unit:]
        for i, s in enumerate(slots):
            self._held[s] = whole[i].clone()
        return out

    @torch.no_grad()
    def push(self, slots, x: torch.Tensor):
        """Feed row i of `x` to `slots[i]` (n distinct open slots); returns n tensors, what each slot releases (possibly nothing)."""
        slots = self._check_push(slots, x)
        if self._rs is None or not self._encode:
            return self._advance(slots, self._plan(slots, [int(x.shape[1])] * len(slots)), list(x))
        plan = self._plan(slots, [self._rs.out_len(s, int(x.shape[1])) for s in slots])
        return self._advance(slots, plan, self._rs.push(slots, x))

    @torch.no_grad()
    def finish(self, slot: int) -> torch.Tensor:
        """Close `slot`'s resampler.  Encode: its tail goes into the slot; returns the tokens [f, K] of the frames that completes (a
        trailing partial frame stays pending).  Decode: returns the tail [m]; with everything `slot` returned before, the signal has
        `toks_to_sig`'s length (held warm-up frames are not decoded).  Nothing on a pool without a resampler.  Afterwards the slot
        accepts only `close`."""
        slot = self._unfinished("finish", self._slot(slot))
        out = self._output(0)
        if self._rs is not None and self._encode:
            plan = self._plan([slot], [self._rs.out_len(slot, 0, True)])
            out = self._advance([slot], plan, self._rs.push([slot], self._no_input(1), finish=True))[0]
        elif self._rs is not None:
            out = self._rs.push([slot], torch.empty(1, 0, dtype=torch.float32, device=self.device), finish=True)[0]
        self._done[slot] = True
        return out
