"""The per-slot resampler on the GPU: alone (audiocodecs_amd.ResampleSlots, ac_resample_stream_*_slots) and inside the session pools
(`encode_sessions` / `decode_sessions(..., resample=True)`).

The contract is the lone stream's, per slot: a slot's pushes and its closing push are `torch.equal` to `resample` on its whole signal,
whichever slot it sits in, whatever the other rows of its calls carry and however many calls it sits out; against the fp64 oracle
the bars are those of tests/test_resample_stream_gpu.py (2e-6 at 16 <-> 24 kHz, 3e-5 with 44.1 kHz: the same chain per output).
Inside the codecs every session of a resampling pool is compared bitwise with a lone resampling stream of batch 1 fed the same
pieces."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from encodec_stream_cases import HOP as E_HOP
from golden_cases import noise
from mimi_stream_cases import HOP as M_HOP
from oracle import resample_oracle as R
from test_resample_stream_gpu import FRAMES, RATES, cycled, encodecs, mimis, sizes_16k  # noqa: F401 (encodecs, mimis: fixtures)

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_ENOMEM = -1, -3
CAP, T = 5, 5003
SLOT_OF = [3, 0, 4, 1, 2]          # session j sits in slot SLOT_OF[j]
STARTS = [0, 2, 3, 5, 8]           # ... and starts at this call: the counts of one call differ, mod o too
CYCLE = (7, 0, 213, 1, 320, 2, 900)   # one sample, nothing, shorter than the history (taps - 1 = 474 at 44.1 -> 16 kHz) and longer

_WHOLE = {}


def whole(rates):
    """(x on the device, the one-shot kernel's result, the fp64 oracle's): computed once per rate pair and left unchanged."""
    from audiocodecs_amd.resample import resample

    if rates not in _WHOLE:
        x = noise(72, CAP, T, amp=0.3)
        _WHOLE[rates] = (x.cuda(), resample(x.cuda(), *rates), R.resample(x.numpy(), *rates))
    return _WHOLE[rates]


def drive(rs, x, restart=None):
    """Feed session j its row of x on a ragged schedule: one call per tick for every live session that still has the tick's L samples
    (slots listed in descending order), session 1 sitting out two ticks in five; a session with fewer left closes alone, with what it
    has, while the others go on.  `restart` = (session, tick): that session's slot restarts alone and its signal starts over.
    Returns (per session the concatenated output, what the schedule covered)."""
    S = x.shape[0]
    pos, outs, done = [0] * S, [[] for _ in range(S)], [False] * S
    seen = dict(phases=0, lens=0, closing_with_data=0, closing_empty=0, sat_out=0)
    t = 0
    while not all(done):
        for j in range(S):
            if t == STARTS[j]:
                rs.restart([SLOT_OF[j]])
        if restart is not None and t == restart[1]:
            j = restart[0]
            assert 0 < pos[j] < T and not done[j]
            rs.restart([SLOT_OF[j]])
            assert rs.consumed[SLOT_OF[j]] == rs.emitted[SLOT_OF[j]] == 0
            pos[j], outs[j] = 0, []
        L = CYCLE[t % len(CYCLE)]
        live = [j for j in range(S) if STARTS[j] <= t and not done[j]]
        seen["sat_out"] += 1 in live and t % 5 in (3, 4)
        live = [j for j in live if not (j == 1 and t % 5 in (3, 4))]
        full = sorted((j for j in live if T - pos[j] >= L), key=lambda j: -SLOT_OF[j])
        if full:
            slots = [SLOT_OF[j] for j in full]
            want = [rs.out_len(s, L) for s in slots]
            seen["phases"] += len({rs.consumed[s] % rs.o for s in slots}) > 1
            seen["lens"] += len(set(want)) > 1
            res = rs.push(slots, torch.stack([x[j, pos[j]:pos[j] + L] for j in full], 0))
            for j, s, y, m in zip(full, slots, res, want):
                assert y.dtype == torch.float32 and y.shape == (m,) and m % rs.n == 0
                outs[j].append(y)
                pos[j] += L
                assert rs.consumed[s] == pos[j]
        for j in live:
            if j not in full:                                # fewer than L left: the closing push brings them
                s = SLOT_OF[j]
                m = rs.out_len(s, T - pos[j], True)
                y, = rs.push([s], x[j:j + 1, pos[j]:], finish=True)
                seen["closing_with_data" if T > pos[j] else "closing_empty"] += 1
                assert y.shape == (m,) and rs.consumed[s] == T and rs.emitted[s] == math.ceil(rs.n * T / rs.o)
                outs[j].append(y)
                pos[j], done[j] = T, True
        t += 1
    return [torch.cat(o) for o in outs], seen


# ---- 1. the resampler alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_every_slot_is_bit_equal_to_the_one_shot_kernel(rates):
    from audiocodecs_amd import ResampleSlots

    x, one_shot, ref64 = whole(rates)
    rs = ResampleSlots(*rates, CAP)
    assert rs.latency_samples == rs.width + rs.o - 1 and rs.taps == 2 * rs.width + rs.o and rs.capacity == CAP
    got, seen = drive(rs, x)
    assert seen["phases"] >= 5 and seen["lens"] >= 5 and seen["closing_with_data"] >= 1 and seen["sat_out"] >= 4, seen
    for j in range(CAP):
        assert got[j].shape == one_shot[j].shape == (math.ceil(rs.n * T / rs.o),)
        assert torch.equal(got[j], one_shot[j]), f"session {j} (slot {SLOT_OF[j]})"
        err = float(np.abs(got[j].cpu().numpy() - ref64[j]).max())
        print(f"resample_slots {rates} session {j}: max error against fp64 {err:.3e}")
        assert err < (2e-6 if max(rates) == 24000 else 3e-5)
    with pytest.raises(ValueError, match="finish"):
        rs.push([SLOT_OF[0]], x[:1, :10])
    rs.restart([SLOT_OF[0]])                                 # a closed slot comes back through restart, alone
    y = torch.cat(rs.push([SLOT_OF[0]], x[2:3, :700]) + rs.push([SLOT_OF[0]], x[2:3, 700:1000], finish=True))
    from audiocodecs_amd.resample import resample
    assert torch.equal(y, resample(x[2:3, :1000].contiguous(), *rates)[0])


def test_a_slot_restarted_alone_starts_over_and_the_others_run_on():
    from audiocodecs_amd import ResampleSlots

    rates = (44100, 16000)
    x, one_shot, _ = whole(rates)
    got, _ = drive(ResampleSlots(*rates, CAP), x, restart=(3, 12))
    for j in range(CAP):
        assert torch.equal(got[j], one_shot[j]), f"session {j}"


@pytest.mark.parametrize("rates", [(16000, 24000), (44100, 16000)], ids=lambda r: f"{r[0]}to{r[1]}")
def test_a_nan_fed_slot_leaves_its_neighbours_bitwise_unchanged(rates):
    from audiocodecs_amd import ResampleSlots

    x, one_shot, _ = whole(rates)
    bad = x.clone()
    bad[1] = float("nan")
    got, _ = drive(ResampleSlots(*rates, CAP), bad)
    assert bool(torch.isnan(got[1]).all()) and got[1].shape == one_shot[1].shape
    for j in (0, 2, 3, 4):
        assert torch.equal(got[j], one_shot[j]), f"session {j}"


# ---- 2. the C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_errors_leave_the_state_usable():
    from audiocodecs_amd import _native
    from audiocodecs_amd.resample import sinc_kernel

    rates = (16000, 24000)
    x, one_shot, _ = whole(rates)
    lib = _native.lib()
    kern, n, o, width = sinc_kernel(*rates)
    kern, taps = kern.cuda(), kern.shape[1]
    H, L = taps - 1, 500
    nbytes = lib.ac_resample_stream_state_bytes(CAP, taps)
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=x.device)
    off = (-buf.data_ptr()) % 256
    state = buf[off:off + nbytes]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    m0 = lib.ac_resample_stream_out_len(0, L, n, o, width, 0)
    wide = m0 + 8 * n
    y = torch.zeros(3, wide, device=x.device)
    xin = x[:3, :L].contiguous()

    def push(slots, counts, dev_slots=None, dev_counts=None, st=state, sb=nbytes, b=CAP, ll=L, tt=taps, ww=width, xp=L, yp=wide, cap=wide, fin=0,
             src=xin, dst=y):
        r = len(slots)
        ds = torch.tensor(slots if dev_slots is None else dev_slots, dtype=torch.int32, device=x.device)
        dc = torch.tensor(counts if dev_counts is None else dev_counts, dtype=torch.int64, device=x.device)
        return lib.ac_resample_stream_push_slots(ptr(st), sb, b, (C.c_int * r)(*slots), (C.c_longlong * r)(*counts), ptr(ds), ptr(dc), r, ptr(src), xp, ll,
                                                 ptr(kern), n, o, tt, ww, ptr(dst), yp, cap, fin, stream)

    def reset_slots(slots, dev_slots=None, st=state, sb=nbytes, b=CAP, tt=taps, ww=width):
        r = len(slots)
        ds = torch.tensor(slots if dev_slots is None else dev_slots, dtype=torch.int32, device=x.device)
        return lib.ac_resample_stream_reset_slots(ptr(st), sb, b, n, o, tt, ww, (C.c_int * r)(*slots), ptr(ds), r, stream)

    assert lib.ac_resample_stream_reset(ptr(state), nbytes, CAP, n, o, taps, width, stream) == 0
    torch.cuda.synchronize()
    fresh = state.clone()
    # refused on the host: nothing is launched
    assert push([4, 4, 1], [0, 0, 0]) == AC_EINVAL and push([4, CAP, 1], [0, 0, 0]) == AC_EINVAL and push([4, -1, 1], [0, 0, 0]) == AC_EINVAL
    assert push([4, 2, 1], [0, -1, 0]) == AC_EINVAL                                  # a negative count
    assert push([4, 2, 1], [0, 0, 0], tt=taps + 1) == AC_EINVAL and push([4, 2, 1], [0, 0, 0], ww=width + 1) == AC_EINVAL
    assert push([4, 2, 1], [0, 0, 0], xp=L - 1) == AC_EINVAL and push([4, 2, 1], [0, 0, 0], yp=m0 - 1) == AC_EINVAL
    assert push([4, 2, 1], [0, 0, 0], ll=-1) == AC_EINVAL and push([4, 2, 1], [0, 0, 0], st=buf[off + 4:]) == AC_EINVAL
    assert push([4, 2, 1], [0, 0, 0], sb=nbytes - 256) == AC_ENOMEM and push([4, 2, 1], [0, 0, 0], cap=m0 - 1) == AC_ENOMEM
    assert reset_slots([1, 1]) == AC_EINVAL and reset_slots([CAP]) == AC_EINVAL and reset_slots([-1]) == AC_EINVAL
    assert reset_slots([1], tt=taps + 1) == AC_EINVAL and reset_slots([1], sb=nbytes - 256) == AC_ENOMEM
    torch.cuda.synchronize()
    assert bool((y == 0).all()) and torch.equal(state, fresh)
    # ... and the state still works: rows 0, 1, 2 of x to slots 4, 2, 1
    assert push([4, 2, 1], [0, 0, 0]) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[:, :m0], one_shot[:3, :m0]) and bool((y[:, m0:] == 0).all())            # behind m_r: untouched
    warm = state.clone()
    # a stale count for one row: that row NaN and its state as it was; the other rows come out right, each at its own length
    m1 = lib.ac_resample_stream_out_len(L, L, n, o, width, 0)
    stale = L - 2
    ms = lib.ac_resample_stream_out_len(stale, L, n, o, width, 0)
    assert max(ms, m1) <= wide
    y.zero_()
    nxt = x[:3, L:2 * L].contiguous()
    assert push([4, 2, 1], [L, stale, L], src=nxt) == 0
    torch.cuda.synchronize()
    assert torch.equal(y[0, :m1], one_shot[0, m0:m0 + m1]) and torch.equal(y[2, :m1], one_shot[2, m0:m0 + m1])
    assert bool(torch.isnan(y[1, :ms]).all()) and bool((y[1, ms:] == 0).all()) and bool((y[0, m1:] == 0).all())
    y.zero_()
    assert push([2], [L], src=nxt[1:2], dst=y[1:2]) == 0                              # slot 2 had not moved
    torch.cuda.synchronize()
    assert torch.equal(y[1, :m1], one_shot[1, m0:m0 + m1])
    # a device list whose copy holds an out-of-range entry: that row NaN, no write anywhere in the state
    for wrong in (CAP, -1, 1 << 30):
        before = state.clone()
        y.zero_()
        assert push([3], [0], dev_slots=[wrong], src=xin[:1], dst=y[:1]) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(y[0, :m0]).all()) and bool((y[0, m0:] == 0).all()) and bool((y[1:] == 0).all()) and torch.equal(state, before)
        assert reset_slots([3], dev_slots=[wrong]) == 0
        torch.cuda.synchronize()
        assert torch.equal(state, before)
    before = state.clone()
    y.zero_()
    assert push([3], [0], dev_counts=[-1], src=xin[:1], dst=y[:1]) == 0                # a device count that is no count
    assert reset_slots([1], b=CAP - 1) == 0                                            # not this state's header: nothing happens
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[0, :m0]).all()) and bool((y[0, m0:] == 0).all()) and torch.equal(state, before)
    # reset_slots writes the listed slot's count and history and nothing else
    assert reset_slots([2]) == 0
    torch.cuda.synchronize()
    hist0 = 256 + (8 * CAP + 255) // 256 * 256
    want = before.clone()
    want[256 + 8 * 2:256 + 8 * 3] = 0
    want[hist0 + 4 * H * 2:hist0 + 4 * H * 3] = 0
    assert torch.equal(state, want) and not torch.equal(state, before) and not torch.equal(warm, fresh)
    # a closing push on slot 4 while slot 1 continues; afterwards slot 4 answers NaN until it is restarted
    tail = lib.ac_resample_stream_out_len(2 * L, 0, n, o, width, 1)
    yt = torch.zeros(1, tail + n, device=x.device)
    from audiocodecs_amd.resample import resample
    assert push([4], [2 * L], ll=0, fin=1, src=xin[:1], dst=yt, yp=tail + n, cap=tail + n) == 0
    torch.cuda.synchronize()
    assert torch.equal(yt[0, :tail], resample(x[:1, :2 * L].contiguous(), *rates)[0, m0 + m1:])
    y.zero_()
    assert push([4, 1], [2 * L, 2 * L], src=x[:2, :L].contiguous(), dst=y[:2]) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[0, :m1]).all()) and not bool(torch.isnan(y[1, :m1]).any())


# ---- 3. inside the session pools ----------------------------------------------------------------------------------------------------
POOL_STARTS = [0, 3, 5]


def staggered(pool, lone_of, rows, sizes, unit_rows):
    """Session j opens at tick POOL_STARTS[j]; every tick is ONE pool push of sizes[t] units for all live sessions, each from its own
    row.  Every session is shadowed by a lone stream of batch 1 fed the same pieces; both are closed with `finish` at the end.
    Returns per session (pool result, lone result), concatenated."""
    slot, lone, pos, got, want = {}, {}, [0] * len(rows), [[] for _ in rows], [[] for _ in rows]
    for t, n in enumerate(sizes):
        for j, s0 in enumerate(POOL_STARTS):
            if t == s0:
                slot[j], lone[j] = pool.open(), lone_of()
        live = [j for j in range(len(rows)) if POOL_STARTS[j] <= t]
        res = pool.push([slot[j] for j in live], torch.stack([rows[j][pos[j]:pos[j] + n] for j in live], 0))
        for j, r in zip(live, res):
            got[j].append(r)
            want[j].append(lone[j].push(rows[j][None, pos[j]:pos[j] + n])[0])
            assert r.shape == want[j][-1].shape, (t, j)
            pos[j] += n
    assert [slot[j] for j in range(len(rows))] == [0, 1, 2]
    for j in (1, 0, 2):                                      # sessions close one by one; the others stay open
        got[j].append(pool.finish(slot[j]))
        want[j].append(lone[j].finish()[0])
        with pytest.raises(ValueError, match="finish"):
            pool.push([slot[j]], rows[j][None, :unit_rows])
        with pytest.raises(ValueError, match="finish"):
            pool.finish(slot[j])
    return [torch.cat(g, 0) for g in got], [torch.cat(w, 0) for w in want], slot, pos


@pytest.mark.parametrize("which", ["encodec", "mimi"])
def test_encode_sessions_resample_like_lone_streams(which, request):
    cfg, sd, c16, c24 = request.getfixturevalue("encodecs" if which == "encodec" else "mimis")
    hop = E_HOP if which == "encodec" else M_HOP
    total, sizes = sizes_16k(hop, (7, 0, 213, 1, 320, 2, 900) if which == "encodec" else (7, 0, 213, 1, 1280, 2, 2900))
    sig = noise(711, 3, total).cuda()
    pool = c16.encode_sessions(4, resample=True)
    got, want, slot, pos = staggered(pool, lambda: c16.encode_stream(1, resample=True), list(sig), sizes, 5)
    assert pos[0] == total and pos[2] < pos[1] < total
    for j in range(3):
        assert got[j].dtype == torch.int64 and got[j].shape == want[j].shape and torch.equal(got[j], want[j]), f"session {j}"
        emitted = math.ceil(3 * pos[j] / 2)                                            # frames and the rest count resampled samples
        assert got[j].shape[0] == pool.frames(slot[j]) and pool.frames(slot[j]) * hop + pool.pending(slot[j]) == emitted
        assert pool._rs.consumed[slot[j]] == pos[j] and pool._rs.emitted[slot[j]] == emitted
    assert got[0].shape[0] == FRAMES
    pool.close(1)
    assert pool.open() == 1 and pool._rs.consumed[1] == 0 and pool.pending(1) == 0           # `open` restarts the resampler slot too
    lone = c16.encode_stream(1, resample=True)
    again = torch.cat([pool.push([1], sig[1:2, :pos[1]])[0], pool.finish(1)], 0)
    assert again.shape[0] > 0 and torch.equal(again, torch.cat([lone.push(sig[1:2, :pos[1]]), lone.finish()], 1)[0])


@pytest.mark.parametrize("which", ["encodec", "mimi"])
def test_decode_sessions_resample_like_lone_streams(which, request):
    from audiocodecs_amd import prng

    cfg, sd, c16, c24 = request.getfixturevalue("encodecs" if which == "encodec" else "mimis")
    K = c16.num_codebooks
    toks = torch.from_numpy(prng.randint(712, "rslots", (3, FRAMES, K), c16.vocab_size)).to(torch.int64).cuda()
    sizes = cycled((1, 0, 3, 2, 7), FRAMES)
    pool = c16.decode_sessions(4, resample=True)
    got, want, slot, pos = staggered(pool, lambda: c16.decode_stream(1, resample=True), list(toks), sizes, 1)
    assert pos[0] == FRAMES and pos[2] < pos[1] < FRAMES
    for j in range(3):
        assert got[j].dtype == torch.float32 and got[j].shape == want[j].shape and torch.equal(got[j], want[j]), f"session {j}"
        frames = pool.frames(slot[j])                                                   # (EnCodec: a short session may still sit in its hold)
        assert got[j].shape[0] == (c16.toks_to_sig(toks[j:j + 1, :frames]).shape[1] if frames else 0)
    assert pool.frames(slot[0]) == FRAMES and pool.frames(slot[1]) > 0


@pytest.mark.parametrize("which", ["encodec", "mimi"])
def test_keyword_behaviour(which, request):
    cfg, sd, c16, c24 = request.getfixturevalue("encodecs" if which == "encodec" else "mimis")
    hop = c24.config.hop_length
    for fn in (c16.encode_sessions, c16.decode_sessions):    # the default keyword at another rate: refused as before, naming the opt-in
        with pytest.raises(ValueError, match="resample=True"):
            fn(2)
        with pytest.raises(TypeError):
            fn(2, None, True)                                # keyword-only
    sig = noise(713, 2, 9 * hop + 11).cuda()
    a, b = c24.encode_sessions(2, resample=True), c24.encode_sessions(2)      # equal rates: the plain pool
    assert a._rs is None and [a.open(), a.open(), b.open(), b.open()] == [0, 1, 0, 1]
    for lo, hi in ((0, 100), (100, 8 * hop), (8 * hop, sig.shape[1])):
        for x, y in zip(a.push([1, 0], sig[:, lo:hi]), b.push([1, 0], sig[:, lo:hi])):
            assert torch.equal(x, y)
    assert a.finish(0).shape == (0, c24.num_codebooks) and a.pending(0) == b.pending(0) == 11
    with pytest.raises(ValueError, match="finish"):
        a.push([0], sig[:1, :5])
    assert a.push([1], sig[:1, :hop])[0].shape[0] == 1       # its neighbour runs on
