"""The grouping rule of a session pool (Encodec.encode_sessions / decode_sessions; Mimi.encode_sessions /
decode_sessions, section 8g, with warmup = 1: Mimi pads with zeros and holds nothing back), as a pure function.

A pool serves sessions that begin and end at different times on one stream state.  Every slot follows the rule a whole lockstep
stream follows (encodec.py `EncodecEncodeStream._take` / `EncodecDecodeStream._decode`): units that do not fill a frame wait, and a
slot that has run nothing yet holds until `warmup` whole frames are in and then releases them all in one go.  The native push runs
the same number of frames for every row it is given, so the rows of one `push` are grouped by the number of frames they run: one
native call per group, the groups in ascending F.  Nothing here needs a GPU (tests/test_encodec_sessions.py)."""

from __future__ import annotations

from typing import List, Sequence, Tuple

__all__ = ["plan_push"]


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
