"""The host logic of the lockstep stream (audiocodecs_amd/streams.py `LockstepStream`) and the session pool (sessions.py `SessionPool`)
on CPU tensors: hold, group, release and refuse, with a toy backend in place of the library.  No GPU and no shared library are needed.

The toy codec (hop 4, K 2) keeps two numbers per slot, the frames run since its restart and a running checksum, so a frame's result
depends on where the slot stands and on everything it ran before: a push that reached the wrong slot, ran in the wrong order or twice
shows in every later frame.  The backend asserts what the native side enforces (distinct slots in range, one F per call, a fresh slot's
first run brings the warm-up).  Two flavours: EnCodec-like (warm-up 7, lockstep streams reset together, no position limit) and Mimi-like
(warm-up 1, single slots restart, a position limit).  The schedules run far below the Mimi-like limit; the refusal tests reach it by
lowering `MAX_POSITIONS` on the instance for one call, as tests/test_mimi_sessions_gpu.py does with the real pools.

The toy classes are built the way the eight public ones are (encodec.py `_OnEncodec`, mimi.py `_OnMimi`): a mixin that makes the
backend and hands `*resample` on, in front of `LockstepStream` or `SessionPool`, with the public aliases `pending` / `pending_frames`,
`frames` and `WARMUP_FRAMES`; the tests read those."""

import random
from types import SimpleNamespace

import pytest
import torch

from audiocodecs_amd.sessions import SessionPool, plan_push
from audiocodecs_amd.streams import LockstepStream

HOP, K = 4, 2
CODEC = SimpleNamespace(sample_rate=24000, config=SimpleNamespace(sampling_rate=24000))
FLAVOURS = {"encodec_like": dict(warmup=7, together="toy streams reset together (`streams` must be None)", limit=None),
            "mimi_like": dict(warmup=1, together=None, limit=2 * 5000)}      # (stride 2: 5000 frames, far above what the schedules run)


def toy_codec(kind, x, ran=0, chk=0):
    """One row through the toy codec from the slot state (ran, chk): [F * HOP] fp32 -> [F, K] int64, or [F, K] int64 -> [F * HOP] fp32.
    Returns (result, ran, chk)."""
    rows = []
    if kind == "encode":
        for f, total in enumerate(x.view(-1, HOP).sum(1).round().to(torch.int64).tolist()):
            chk = (chk * 31 + total) % 9973
            rows.append((ran + f, chk))
        return torch.tensor(rows, dtype=torch.int64).view(-1, K), ran + len(rows), chk
    for f, total in enumerate(x.sum(1).tolist()):
        chk = (chk * 31 + total) % 9973
        rows.append([j + 8.0 * (ran + f) + chk / 16.0 for j in range(HOP)])
    return torch.tensor(rows, dtype=torch.float32).view(-1), ran + len(rows), chk


class ToyBackend:
    """The backend interface of streams.py on a CPU state tensor: int64 [n][2] = (frames since restart, checksum) per slot."""

    device = torch.device("cpu")
    hop, stride = HOP, 2

    def __init__(self, kind, warmup, together):
        self.kind, self.warmup, self.reset_together = kind, warmup, together
        self.calls = []        # (F, slots) of every run, in order

    def _slots(self, state, n):
        return state.view(torch.int64).view(n, 2)

    def state_bytes(self, n):
        return 16 * n

    def reset(self, state, n, mask=None):
        assert mask is None
        self._slots(state, n).zero_()

    def restart_slots(self, state, cap, slots):
        assert len(set(slots)) == len(slots) and all(0 <= s < cap for s in slots)
        self._slots(state, cap)[list(slots)] = 0

    def workspace_bytes(self, n, F):
        return 64 * n * F

    def run(self, state, cap, slots, src, F, nK, dst, ws):
        rows = list(range(cap)) if slots is None else list(slots)
        assert len(set(rows)) == len(rows) and all(type(s) is int and 0 <= s < cap for s in rows)
        assert nK == K and F >= 1 and ws.numel() >= self.workspace_bytes(len(rows), F)
        assert src.is_contiguous() and tuple(src.shape) == ((len(rows), F * HOP) if self.kind == "encode" else (len(rows), F, K))
        st = self._slots(state, cap)
        for j, s in enumerate(rows):
            ran, chk = int(st[s, 0]), int(st[s, 1])
            assert ran > 0 or F >= self.warmup, f"slot {s}: a fresh slot's first run brings {F} frames, fewer than the warm-up"
            dst[j], ran, chk = toy_codec(self.kind, src[j], ran, chk)
            st[s, 0], st[s, 1] = ran, chk
        self.calls.append((F, rows))


class _OnToy:
    """The toy side of the four classes below, shaped like `_OnEncodec` / `_OnMimi`."""

    def __init__(self, flavour, n, *resample):
        f = FLAVOURS[flavour]
        be = ToyBackend(self._kind, f["warmup"], f["together"])
        self.WARMUP_FRAMES = be.warmup
        super().__init__(CODEC, be, n, K, *resample)
        if f["limit"] is not None:
            self.MAX_POSITIONS = f["limit"]


class ToyEncodeStream(_OnToy, LockstepStream):
    _kind = "encode"
    pending = LockstepStream._waiting
    frames = property(lambda self: self._frames[0])


class ToyDecodeStream(_OnToy, LockstepStream):
    _kind = "decode"
    pending_frames = LockstepStream._waiting
    frames = ToyEncodeStream.frames


class ToyEncodeSessions(_OnToy, SessionPool):
    _kind = "encode"


class ToyDecodeSessions(_OnToy, SessionPool):
    _kind = "decode"


def make(what, flavour, kind, n):
    if what == "pool":
        return (ToyEncodeSessions if kind == "encode" else ToyDecodeSessions)(flavour, n)
    return (ToyEncodeStream if kind == "encode" else ToyDecodeStream)(flavour, n, False)


def waiting(s):
    return s.pending if s._encode else s.pending_frames


def payload(rng, kind, rows, units):
    g = torch.Generator().manual_seed(rng.randrange(1 << 30))
    if kind == "encode":
        return torch.randint(-50, 50, (rows, units), generator=g).float()
    return torch.randint(0, 1000, (rows, units, K), generator=g)


def sizes(kind, warmup):
    """Piece lengths in units: nothing, one, a frame less one, a frame, ragged, and more than the warm-up in one go."""
    if kind == "encode":
        return [0, 1, HOP - 1, HOP, HOP + 1, 3 * HOP + 2, warmup * HOP - 1, warmup * HOP + 3, (warmup + 2) * HOP]
    return [0, 1, 1, 2, 3, warmup - 1, warmup, warmup + 2]


BOTH = pytest.mark.parametrize("kind", ["encode", "decode"])
FLAV = pytest.mark.parametrize("flavour", list(FLAVOURS))


# ---- 1. a lone stream ----------------------------------------------------------------------------------------------------------------
@FLAV
@BOTH
def test_lone_stream_in_random_pieces_is_the_one_shot_result(flavour, kind):
    rng = random.Random(f"lone/{flavour}/{kind}")
    warmup, unit, B = FLAVOURS[flavour]["warmup"], HOP if kind == "encode" else 1, 2
    s = make("stream", flavour, kind, B)
    pieces = [rng.choice(sizes(kind, warmup)) for _ in range(60)] + sizes(kind, warmup)
    whole = payload(rng, kind, B, sum(pieces))
    got, at, pend, ran = [], 0, 0, 0
    for L in pieces:
        out = s.push(whole[:, at:at + L].contiguous())
        at += L
        n = (pend + L) // unit                               # the per-row rule, restated
        n = 0 if (ran == 0 and n < warmup) else n
        pend, ran = pend + L - n * unit, ran + n
        assert out.shape[1] == (n if kind == "encode" else n * HOP) and out.dtype == (torch.int64 if kind == "encode" else torch.float32)
        assert waiting(s) == pend and s.frames == ran and s._frames == [ran] * B
        got.append(out)
    got = torch.cat(got, 1)
    assert ran > 3 * warmup and s._be.calls and all(rows == [0, 1] for _, rows in s._be.calls)
    for b in range(B):
        want, _, _ = toy_codec(kind, whole[b, : ran * unit])
        assert torch.equal(got[b], want)
    assert s.finish().shape[1] == 0 and waiting(s) == pend and s.WARMUP_FRAMES == warmup and s._rs is None


# ---- 2. a pool against lone streams --------------------------------------------------------------------------------------------------
def run_schedule(flavour, kind, steps, tamper=None):
    """A seeded schedule of open / close / push on a pool of 5, every session shadowed by a lone stream of batch 1 fed the same pieces.
    `tamper(pool, rng)`, called before every step, may try what the pool must refuse.  Returns what the schedule covered."""
    rng = random.Random(f"pool/{flavour}/{kind}")
    warmup, unit = FLAVOURS[flavour]["warmup"], HOP if kind == "encode" else 1
    pool = make("pool", flavour, kind, 5)
    lone, opened, mixed, pushes = {}, [0] * 5, 0, 0
    for step in range(steps):
        if tamper is not None:
            tamper(pool, random.Random(step))
        assert pool.active == sorted(lone)
        r = rng.random()
        p_open, p_close = (0.4, 0.05) if (step // 20) % 2 == 0 else (0.05, 0.3)     # the pool fills and drains in turn: every slot comes round
        if (r < p_open or not lone) and len(lone) < 5:
            slot = pool.open()
            assert slot == min(set(range(5)) - set(lone)) and pool.frames(slot) == 0 and pool.pending(slot) == 0
            lone[slot] = make("stream", flavour, kind, 1)
            opened[slot] += 1
        elif r < p_open + p_close and lone:
            slot = rng.choice(sorted(lone))
            pool.close(slot)
            del lone[slot]
        else:
            slots = rng.sample(sorted(lone), rng.randint(1, len(lone)))
            x = payload(rng, kind, len(slots), rng.choice(sizes(kind, warmup)))
            want_plan = plan_push([pool.pending(s) for s in slots], [pool.frames(s) for s in slots], [x.shape[1]] * len(slots), unit, warmup)
            fresh = [pool.frames(s) == 0 for s in slots]
            before = len(pool._be.calls)
            got = pool.push(slots, x)
            assert pool._be.calls[before:] == [(F, [slots[i] for i in rows]) for F, rows in want_plan]
            ran_rows = {i for _, rows in want_plan for i in rows}
            mixed += any(fresh[i] for i in ran_rows) and any(not fresh[i] for i in ran_rows)
            pushes += 1
            for i, slot in enumerate(slots):
                want = lone[slot].push(x[i:i + 1].contiguous())[0]
                assert got[i].dtype == want.dtype and torch.equal(got[i], want), (step, slot)
                assert pool.frames(slot) == lone[slot].frames and pool.pending(slot) == waiting(lone[slot])
    return SimpleNamespace(opened=opened, mixed=mixed, pushes=pushes, pool=pool)


@FLAV
@BOTH
def test_pool_sessions_match_lone_streams_bit_for_bit(flavour, kind):
    seen = run_schedule(flavour, kind, 260)
    assert min(seen.opened) >= 3, seen.opened                # every slot reopened at least twice
    assert seen.mixed >= 1 and seen.pushes >= 100            # a fresh slot and warm ones in one push; most steps are pushes


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
@FLAV
@BOTH
def test_pool_refusals_leave_the_schedule_on_track(flavour, kind):
    tried = set()

    def tamper(pool, rng):
        def snapshot():
            return pool.active, [pool.pending(s) for s in pool.active], [pool.frames(s) for s in pool.active], len(pool._be.calls)

        def refused(what, match, fn, *args):
            was = snapshot()
            with pytest.raises(ValueError, match=match):
                fn(*args)
            assert snapshot() == was
            tried.add(what)

        act, closed = pool.active, sorted(set(range(5)) - set(pool.active))
        if not closed:
            refused("full", "full", pool.open)
        if not act:
            return
        a = act[0]
        one = payload(rng, kind, 1, 2 * (HOP if kind == "encode" else 1))
        two = torch.cat([one, one], 0)
        refused("twice", "twice", pool.push, [a, a], two)
        if closed:
            refused("closed", "not open", pool.push, [a, closed[0]], two)
            refused("closed", "not open", pool.close, closed[0])
            refused("closed", "not open", pool.frames, closed[0])
        refused("range", "outside", pool.push, [a, 5], two)
        refused("range", "outside", pool.push, [a, -1], two)
        refused("bool", "outside", pool.push, [a, True], two)
        refused("sequence", "sequence", pool.push, a, one)
        refused("rows", "expects", pool.push, [a], two)
        refused("dtype", "expects", pool.push, [a], one.double() if kind == "encode" else one.int())
        refused("rank", "expects", pool.push, [a], one[0])
        refused("rank", "expects", pool.push, [a], one[:, None])
        if kind == "decode":
            refused("K", "expects", pool.push, [a], one[:, :, :1])
        if FLAVOURS[flavour]["limit"] is not None:
            limit, pool.MAX_POSITIONS = pool.MAX_POSITIONS, 2 * (pool.frames(a) + 1)      # one more frame fits, the two of `one` do not
            refused("positions", "positions", pool.push, [a], one)
            pool.MAX_POSITIONS = limit

    run_schedule(flavour, kind, 200, tamper)                 # (run_schedule asserts every push against its lone stream)
    want = {"full", "twice", "closed", "range", "bool", "sequence", "rows", "dtype", "rank"}
    want |= {"K"} if kind == "decode" else set()
    want |= {"positions"} if FLAVOURS[flavour]["limit"] is not None else set()
    assert tried == want


@FLAV
@BOTH
def test_stream_refusals_leave_the_stream_usable(flavour, kind):
    rng = random.Random(f"refuse/{flavour}/{kind}")
    f, unit, B = FLAVOURS[flavour], HOP if kind == "encode" else 1, 2
    s, clean = make("stream", flavour, kind, B), make("stream", flavour, kind, B)
    whole = payload(rng, kind, B, 3 * f["warmup"] * unit + 2 * unit)
    cut = f["warmup"] * unit + (1 if kind == "encode" else 0)              # encode: a sample of a partial frame is left pending
    first = s.push(whole[:, :cut].contiguous())
    assert torch.equal(first, clean.push(whole[:, :cut].contiguous()))

    def refused(match, fn, *args):
        was = (waiting(s), s.frames, list(s._frames), len(s._be.calls))
        with pytest.raises(ValueError, match=match):
            fn(*args)
        assert (waiting(s), s.frames, list(s._frames), len(s._be.calls)) == was

    rest = whole[:, cut:].contiguous()
    for bad in (rest[:1], rest[0], rest[:, None], rest.double() if kind == "encode" else rest.int()) + ((rest[:, :, :1],) if kind == "decode" else ()):
        refused("expects", s.push, bad)
    if f["together"]:
        refused("together", s.reset, [0])
    else:
        for bad in ([B], [-1], [True], True, [0.0]):
            refused("must list slots", s.reset, bad)
        if kind == "encode":
            refused("pending", s.reset, [0])
        limit, s.MAX_POSITIONS = s.MAX_POSITIONS, 2 * (s.frames + 1)
        refused("positions", s.push, rest)
        s.MAX_POSITIONS = limit
    got = s.push(rest)
    assert torch.equal(got, clean.push(rest)) and got.shape[1] > 0
    for b in range(B):
        want, _, _ = toy_codec(kind, whole[b, : s.frames * unit])
        assert torch.equal(torch.cat([first, got], 1)[b], want)
    s.finish()
    refused("finish", s.push, rest)
    refused("finish", s.finish)
    s.reset()
    assert waiting(s) == 0 and s.frames == 0
    again = torch.cat([s.push(whole[:, :cut].contiguous()), s.push(rest)], 1)
    assert torch.equal(again, torch.cat([first, got], 1))
    if not f["together"]:                                    # a slot restarted alone starts over; its neighbour runs on
        if waiting(s):
            s.push(payload(rng, kind, B, unit - waiting(s)))
        s.reset([1])
        assert s._frames[1] == 0 and s._frames[0] > 0
        more = payload(rng, kind, B, 2 * unit)
        out = s.push(more)
        assert torch.equal(out[1], toy_codec(kind, more[1])[0])
        assert not torch.equal(out[0], toy_codec(kind, more[0])[0])
