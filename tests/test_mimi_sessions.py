"""Session pools on Mimi streams, the part that needs no GPU: the grouping rule (audiocodecs_amd/sessions.py plan_push) with
warmup = 1 -- Mimi pads with zeros, so a fresh slot runs its first whole frame at once -- against a per-row simulation of the rule a
lockstep stream applies to itself (streams.py LockstepStream._take, both directions), and the null-handle answers of the two
slot entry points."""
import ctypes as C

import numpy as np
import pytest

from audiocodecs_amd.sessions import plan_push

AC_EINVAL = -1
HOP = 1920


def take(pending, incoming, hop):
    """One row of `_take`: (frames run by this push, units left pending).  No hold: fresh and warm rows follow the same rule."""
    n = (pending + incoming) // hop
    return n, pending + incoming - n * hop


def check_plan(pending, ran, incoming, hop):
    plan = plan_push(pending, ran, incoming, hop, 1)
    want = [take(p, m, hop)[0] for p, m in zip(pending, incoming)]
    got = [0] * len(pending)
    for F, rows in plan:
        assert F >= 1 and rows and rows == sorted(rows)
        for i in rows:
            assert got[i] == 0, f"row {i} is in two groups"
            got[i] = F
    assert got == want
    fs = [F for F, _ in plan]
    assert fs == sorted(set(fs)), "groups must come in ascending F, one per F"
    return plan


@pytest.mark.parametrize("hop", [HOP, 1])
def test_plan_push_with_no_warmup_matches_the_per_row_rule(hop):
    rng = np.random.default_rng(40 + hop)
    for _ in range(300):
        n = int(rng.integers(1, 12))
        pending = [int(v) for v in rng.integers(0, hop, n)]               # a row holds less than a frame, fresh or warm
        ran = [int(v) for v in rng.integers(0, 3, n) * rng.integers(1, 50, n)]
        incoming = [int(v) for v in rng.integers(0, 6 * hop + 1, n)]
        if rng.integers(0, 4) == 0:
            incoming = [incoming[0]] * n       # what one `push` gives: the same count for every row
        check_plan(pending, ran, incoming, hop)


@pytest.mark.parametrize("hop", [HOP, 1])
def test_plan_push_with_no_warmup_edges(hop):
    h = hop
    # a fresh row with exactly one whole frame runs, beside a warm one: one group
    assert check_plan([0, 0], [0, 9], [h, h], h) == [(1, [0, 1])]
    # rows: fresh, one frame completed by what was pending; fresh, two frames; warm, one frame; fresh, no incoming
    assert check_plan([h - 1, 0, h // 2, 0], [0, 0, 9, 0], [1, 2 * h, h, 0], h) == [(1, [0, 2]), (2, [1])]
    assert plan_push([0, 0], [0, 5], [0, 0], h, 1) == []                     # zero incoming runs nothing
    assert plan_push([], [], [], h, 1) == []
    if h > 1:      # a row with no whole frame is left out, fresh or warm
        assert plan_push([0, 0], [0, 7], [h - 1, h - 1], h, 1) == []
        assert check_plan([h - 2, 0, 1], [0, 0, 4], [1, h, h - 2], h) == [(1, [1])]


def test_slot_entry_points_refuse_a_null_handle():
    from test_native_abi import _built

    L = _built().lib()
    slots = (C.c_int * 1)(0)
    buf = (C.c_char * 64)()
    for fn in (L.ac_mimi_stream_encode_slots, L.ac_mimi_stream_decode_slots):
        assert fn(None, buf, 64, 1, slots, slots, 1, buf, 1, 1, buf, buf, 64, None) == AC_EINVAL
        assert fn(None, buf, 64, 1, None, None, 1, buf, 1, 1, buf, buf, 64, None) == AC_EINVAL
