"""The grouping rule of a session pool (Encodec.encode_sessions / decode_sessions; Mimi.encode_sessions /
decode_sessions, section 8g, with warmup = 1: Mimi pads with zeros and holds nothing back), as a pure function.

A pool serves sessions that begin and end at different times on one stream state.  Every slot follows the rule a whole lockstep
stream follows (streams.py `LockstepStream._take`, one rule for both directions): units that do not fill a frame wait, and a
slot that has run nothing yet holds until `warmup` whole frames are in and then releases them all in one go.  The native push runs
the same number of frames for every row it is given, so the rows of one `push` are grouped by the number of frames they run: one
native call per group, the groups in ascending F.  `SessionPool` is the pool itself, for every codec and both directions; like the
lockstep stream it reaches the library through a backend object only, so nothing here needs a GPU (tests/test_encodec_sessions.py,
tests/test_stream_host.py)."""

from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

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
    whichever slot it sits in and whatever the others do."""

    def __init__(self, codec, backend, capacity: int, num_codebooks: int):
        super().__init__(codec, backend, capacity, num_codebooks)
        self.capacity = capacity
        self._is_open = [False] * capacity
        self._ran = [0] * capacity                  # frames run since the slot was opened
        self._held = [self._no_input()] * capacity   # what waits per slot: [m] samples / [m, K] tokens
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

    def pending(self, slot: int) -> int:
        """Units of `slot` that have not run: samples on the encode side, token frames on the decode side."""
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
        self._is_open[slot] = True
        self._ran[slot] = 0
        self._held[slot] = self._no_input()
        return slot

    def close(self, slot: int) -> None:
        """Free `slot`, dropping what it holds (held warm-up frames included)."""
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
        return slots

    @torch.no_grad()
    def push(self, slots, x: torch.Tensor):
        """Feed row i of `x` to `slots[i]` (n distinct open slots); returns n tensors, what each slot releases (possibly nothing)."""
        slots = self._check_push(slots, x)
        unit = self._unit
        plan = plan_push([int(self._held[s].shape[0]) for s in slots], [self._ran[s] for s in slots], [int(x.shape[1])] * len(slots), unit,
                         self._be.warmup)
        if self.MAX_POSITIONS is not None:
            for F, rows in plan:
                for i in rows:
                    if self._be.stride * (self._ran[slots[i]] + F) > self.MAX_POSITIONS:
                        raise ValueError(f"slot {slots[i]} would pass {self.MAX_POSITIONS} transformer positions: close it and open a new session")
        whole = [torch.cat([self._held[s], x[i]], 0) if self._held[s].shape[0] else x[i] for i, s in enumerate(slots)]
        out = [self._output(0) for _ in slots]
        for F, rows in plan:
            src = torch.stack([whole[i][: F * unit] for i in rows], 0).contiguous()
            dst = self._output(len(rows), F)
            group = [slots[i] for i in rows]
            self._run(group, src, F, dst)
            for j, i in enumerate(rows):
                self._ran[slots[i]] += F
                out[i] = dst[j]
                whole[i] = whole[i][F * unit:]
        for i, s in enumerate(slots):
            self._held[s] = whole[i].clone()
        return out
