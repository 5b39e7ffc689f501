"""Session pools on EnCodec streams, the part that needs no GPU: the grouping rule (audiocodecs_amd/sessions.py plan_push) against
a per-row simulation of the rule a lockstep stream applies to itself (streams.py LockstepStream._take, both directions),
and the null-handle answers of the four slot entry points."""
import ctypes as C

import numpy as np
import pytest

from audiocodecs_amd.sessions import plan_push

AC_EINVAL = -1
WARMUP = 7


def take(pending, ran, incoming, hop, warmup):
    """One row of `_take`: (frames run by this push, units left pending)."""
    n = (pending + incoming) // hop
    if n == 0 or (ran == 0 and n < warmup):
        return 0, pending + incoming
    return n, pending + incoming - n * hop


def check_plan(pending, ran, incoming, hop, warmup):
    plan = plan_push(pending, ran, incoming, hop, warmup)
    want = [take(p, r, m, hop, warmup)[0] for p, r, m in zip(pending, ran, incoming)]
    got = [0] * len(pending)
    seen = set()
    for F, rows in plan:
        assert F >= 1 and rows and rows == sorted(rows)
        for i in rows:
            assert i not in seen, f"row {i} is in two groups"
            seen.add(i)
            got[i] = F
            assert ran[i] > 0 or F >= warmup, f"fresh row {i} in a group of F={F}"
    assert got == want
    fs = [F for F, _ in plan]
    assert fs == sorted(set(fs)), "groups must come in ascending F, one per F"
    return plan


@pytest.mark.parametrize("hop", [320, 1])
def test_plan_push_matches_the_per_row_rule(hop):
    rng = np.random.default_rng(20 + hop)
    for _ in range(300):
        n = int(rng.integers(1, 12))
        pending = [int(v) for v in rng.integers(0, WARMUP * hop, n)]      # a held row has up to warm-up - 1 frames and a partial one
        ran = [int(v) for v in rng.integers(0, 3, n) * rng.integers(1, 50, n)]
        pending = [p if r == 0 else p % hop for p, r in zip(pending, ran)]   # a warm row holds less than a frame
        incoming = [int(v) for v in rng.integers(0, 10 * hop + 1, n)]
        if rng.integers(0, 4) == 0:
            incoming = [incoming[0]] * n       # what one `push` gives: the same count for every row
        check_plan(pending, ran, incoming, hop, WARMUP)


@pytest.mark.parametrize("hop", [320, 1])
def test_plan_push_edges(hop):
    h = hop
    # rows: held and staying held; releasing exactly 7; releasing more than 7; warm, one frame; warm, nothing whole; zero incoming
    pending = [3 * h, 6 * h, 5 * h + h // 2, h // 2, 0, 2 * h]
    ran = [0, 0, 0, 9, 9, 0]
    incoming = [h, h, 4 * h, h, h - 1, 0]
    plan = check_plan(pending, ran, incoming, h, WARMUP)
    assert plan == [(1, [3]), (7, [1]), (9, [2])]      # (hop 1 has no partial frames: h // 2 and h - 1 are 0 there; the plan is the same)
    assert plan_push([0, 0], [0, 5], [0, 0], h, WARMUP) == []                      # zero incoming runs nothing
    assert plan_push([6 * h], [0], [h - 1], h, WARMUP) == []                    # one unit short of the release
    assert plan_push([6 * h], [0], [h], h, WARMUP) == [(7, [0])]
    assert plan_push([6 * h] * 3, [0, 0, 4], [h] * 3, h, WARMUP) == [(7, [0, 1, 2])]   # fresh and warm rows share a group when F allows
    assert plan_push([], [], [], h, WARMUP) == []
    for bad in (([1], [0, 0], [1]), ([-1], [0], [1])):
        with pytest.raises(ValueError):
            plan_push(*bad, h, WARMUP)
    with pytest.raises(ValueError):
        plan_push([0], [0], [1], 0, WARMUP)


def test_slot_entry_points_refuse_a_null_handle():
    from test_native_abi import _built

    L = _built().lib()
    slots = (C.c_int * 1)(0)
    buf = (C.c_char * 64)()
    for fn in (L.ac_encodec_stream_reset_slots, L.ac_encodec_stream_decode_reset_slots):
        assert fn(None, buf, 64, 1, slots, slots, 1, None) == AC_EINVAL
    for fn in (L.ac_encodec_stream_encode_slots, L.ac_encodec_stream_decode_slots):
        assert fn(None, buf, 64, 1, slots, slots, 1, buf, 1, 1, buf, buf, 64, None) == AC_EINVAL
