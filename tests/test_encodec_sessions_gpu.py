"""Session pools on EnCodec streams (Encodec.encode_sessions / decode_sessions, include/audiocodecs_amd.h ac_encodec_stream_*_slots).

A pool runs any subset of the slots of one stream state.  The contract is bitwise: a session gives the bits of a lone
`encode_stream(1)` / `decode_stream(1)` fed the same pieces -- whichever slot it sits in, whoever shares its native call, whatever
the unlisted slots hold -- and n listed slots give the bits of the lockstep stream of batch n.  The lockstep stream's own parity
with the reference is tests/test_encodec_stream_gpu.py; case 6 here runs the reference's fixtures through the pool all the same."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from encodec_stream_cases import ENCODE_FRAMES, HOP, WARMUP, signal_of, tokens_of
from golden_cases import REC_STRIDE, noise
from test_encodec_stream_gpu import AC_EINVAL, AC_ENOMEM, WAVE_BAR, check_tokens, codec_for, codecs, rand_toks  # noqa: F401 (codecs: fixture)
from test_gpu_parity import rms
import parity_record

pytestmark = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def lone(stream, pieces):
    """The concatenated output of a batch-1 lockstep stream fed `pieces` (each one session's piece: [L] samples or [F, K] tokens)."""
    return torch.cat([stream.push(p[None]) for p in pieces], 1)[0]


def run_staggered(pool, starts, pieces):
    """Session j opens at tick starts[j] and is fed pieces[j][i] at tick starts[j] + i; every tick is ONE push of all live sessions.
    Returns (per session: the list of per-tick results, per session: its slot)."""
    ticks = max(s + len(p) for s, p in zip(starts, pieces))
    slot, out = {}, [[] for _ in starts]
    for t in range(ticks):
        for j, s0 in enumerate(starts):
            if t == s0:
                slot[j] = pool.open()
        live = [j for j, s0 in enumerate(starts) if s0 <= t < s0 + len(pieces[j])]
        if not live:
            continue
        res = pool.push([slot[j] for j in live], torch.stack([pieces[j][t - starts[j]] for j in live], 0))
        assert len(res) == len(live)
        for j, r in zip(live, res):
            out[j].append(r)
    return out, slot


def cut(x, size):
    """x [T] or [N, K] -> pieces of `size` units (the last one may be shorter)."""
    return [x[a:a + size] for a in range(0, x.shape[0], size)]


def feed(pool, slots, rows_of_pushes):
    """Push a list of [n, ...] tensors to the same slots; per slot the concatenated result."""
    acc = [[] for _ in slots]
    for x in rows_of_pushes:
        for i, r in enumerate(pool.push(slots, x)):
            acc[i].append(r)
    return [torch.cat(a, 0) for a in acc]


# ---- 1. bitwise against the lone stream, staggered ------------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [HOP, 200])
def test_staggered_encode_sessions_are_the_lone_streams(piece, codecs):
    codec = codecs("full")
    starts, ticks = [0, 5, 9], (20 if piece == HOP else 40)      # (40 ticks of 200 samples: the last session gets past its hold too)
    sig = noise(701, 3, ticks * piece).cuda()
    pieces = [cut(sig[j, : (ticks - s0) * piece], piece) for j, s0 in enumerate(starts)]
    pool = codec.encode_sessions(4)
    assert pool.capacity == 4 and pool.WARMUP_FRAMES == WARMUP and pool.hop == HOP and pool.num_codebooks == 8 and pool.active == []
    out, slot = run_staggered(pool, starts, pieces)
    assert [slot[j] for j in range(3)] == [0, 1, 2] and pool.active == [0, 1, 2]
    if piece == HOP:     # tick 11: b releases its 7 held frames beside a's one frame -- two native calls in one push
        assert [int(r.shape[0]) for r in out[1]] == [0] * 6 + [7] + [1] * 8
        assert [int(r.shape[0]) for r in out[0]] == [0] * 6 + [7] + [1] * 13
    for j in range(3):
        got = torch.cat(out[j], 0)
        want = lone(codec.encode_stream(1), pieces[j])
        assert got.dtype == torch.int64 and got.shape == want.shape and want.shape[0] >= WARMUP
        assert torch.equal(got, want), f"session {j}"
        n = len(pieces[j]) * piece
        assert pool.frames(slot[j]) == n // HOP and pool.pending(slot[j]) == n % HOP


def test_staggered_decode_sessions_are_the_lone_streams(codecs):
    codec = codecs("full")
    starts, ticks = [0, 5, 9], 20
    toks = rand_toks(702, 3, ticks)
    pieces = [cut(toks[j, : ticks - s0], 1) for j, s0 in enumerate(starts)]
    pool = codec.decode_sessions(4)
    out, slot = run_staggered(pool, starts, pieces)
    assert [int(r.shape[0]) for r in out[1]] == [0] * 6 + [7 * HOP] + [HOP] * 8
    for j in range(3):
        got = torch.cat(out[j], 0)
        want = lone(codec.decode_stream(1), pieces[j])
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got, want), f"session {j}"
        assert pool.frames(slot[j]) == ticks - starts[j] and pool.pending(slot[j]) == 0


# ---- 2. same launches, other addresses ------------------------------------------------------------------------------------------------
def test_a_listed_subset_is_the_lockstep_stream_of_its_size(codecs):
    """66 of 70 slots, listed in descending order: past the LSTM step kernel's 64 streams per workgroup with a map that is nowhere the
    identity; the one-frame pushes take the short-chunk staging (L < P at the frame-rate convs)."""
    codec = codecs("tiny")
    n = 66
    sig, toks = noise(703, n, 10 * HOP).cuda(), rand_toks(704, n, 10)
    cuts = [(0, 7), (7, 8), (8, 9), (9, 10)]
    for make_pool, make_stream, x, unit in ((codec.encode_sessions, codec.encode_stream, sig, HOP),
                                            (codec.decode_sessions, codec.decode_stream, toks, 1)):
        pool = make_pool(70)
        opened = [pool.open() for _ in range(n)]
        assert opened == list(range(n))
        slots = opened[::-1]
        pushes = [x[:, a * unit:b * unit].contiguous() for a, b in cuts]
        got = feed(pool, slots, pushes)
        s = make_stream(n)
        want = torch.cat([s.push(p) for p in pushes], 1)
        for i in range(n):
            assert torch.equal(got[i], want[i]), f"row {i} (slot {slots[i]})"


# ---- 3. order and neighbours do not matter --------------------------------------------------------------------------------------------
def test_order_and_neighbours_do_not_matter(codecs):
    codec = codecs("tiny")
    sig, toks = noise(705, 4, 10 * HOP).cuda(), rand_toks(706, 4, 10)
    for make_pool, x, unit in ((codec.encode_sessions, sig, HOP), (codec.decode_sessions, toks, 1)):
        results = {}
        for order in ([3, 0, 2], [0, 2, 3]):
            pool = make_pool(4)
            assert [pool.open() for _ in range(4)] == [0, 1, 2, 3]
            idx = torch.tensor(order, device=x.device)
            pushes = [x[idx, a * unit:b * unit].contiguous() for a, b in ((0, 7), (7, 8), (8, 9), (9, 10))]
            results[tuple(order)] = dict(zip(order, feed(pool, order, pushes)))
        for s in (0, 2, 3):
            assert torch.equal(results[(3, 0, 2)][s], results[(0, 2, 3)][s]), f"slot {s}"
        if unit == HOP:      # (tokens have no NaN: the neighbours of the decode side are covered by the other rows above)
            pool = make_pool(4)
            [pool.open() for _ in range(4)]
            y = x.clone()
            y[0], y[3] = float("nan"), float("nan")
            idx = torch.tensor([0, 2, 3], device=x.device)
            pushes = [y[idx, a * unit:b * unit].contiguous() for a, b in ((0, 7), (7, 8), (8, 9), (9, 10))]
            assert torch.equal(feed(pool, [0, 2, 3], pushes)[1], results[(0, 2, 3)][2])


# ---- 4. unlisted slots are untouched --------------------------------------------------------------------------------------------------
def test_unlisted_slots_are_untouched(codecs):
    codec = codecs("tiny")
    for make_pool, make_stream, x, nb, unit in (
            (codec.encode_sessions, codec.encode_stream, noise(707, 1, 14 * HOP).cuda()[0], noise(708, 2, 60 * HOP).cuda(), HOP),
            (codec.decode_sessions, codec.decode_stream, rand_toks(709, 1, 14)[0], rand_toks(710, 2, 60), 1)):
        pool = make_pool(3)
        a, u, b = pool.open(), pool.open(), pool.open()          # u sits between its neighbours
        pieces = [x[: 3 * unit], x[3 * unit: 7 * unit]] + cut(x[7 * unit:], unit)
        t = [0]

        def neighbours(frames_each):
            for f in frames_each:
                pool.push([a, b], nb[:, t[0] * unit:(t[0] + f) * unit].contiguous())
                t[0] += f

        got = [pool.push([u], pieces[0][None])[0]]
        assert got[0].shape[0] == 0 and pool.pending(u) == 3 * unit
        neighbours([7] + [1] * 20)                               # u is held at 3 frames meanwhile
        assert pool.pending(u) == 3 * unit and pool.frames(u) == 0
        got += [pool.push([u], p[None])[0] for p in pieces[1:4]]
        neighbours([1] * 20)                                     # u is warm meanwhile
        got += [pool.push([u], p[None])[0] for p in pieces[4:]]
        assert pool.frames(u) == 14
        assert torch.equal(torch.cat(got, 0), lone(make_stream(1), pieces))


# ---- 5. reuse -------------------------------------------------------------------------------------------------------------------------
def test_a_reused_slot_starts_from_nothing(codecs):
    codec = codecs("tiny")
    for make_pool, make_stream, x, unit in ((codec.encode_sessions, codec.encode_stream, noise(711, 4, 24 * HOP).cuda(), HOP),
                                            (codec.decode_sessions, codec.decode_stream, rand_toks(712, 4, 24), 1)):
        pool = make_pool(3)
        slots = [pool.open() for _ in range(3)]
        with pytest.raises(ValueError):
            pool.open()
        first = feed(pool, slots, [x[:3, : 7 * unit].contiguous()] + [x[:3, f * unit:(f + 1) * unit].contiguous() for f in range(7, 12)])
        pool.close(1)
        assert pool.active == [0, 2]
        assert pool.open() == 1 and pool.frames(1) == 0 and pool.pending(1) == 0
        newcomer = x[3, : 12 * unit]                             # the new session (row 3 of x, from its start) takes slot 1
        rest, new = [[], []], []
        for f in range(12):
            rows = torch.stack([x[0, (12 + f) * unit:(13 + f) * unit], newcomer[f * unit:(f + 1) * unit], x[2, (12 + f) * unit:(13 + f) * unit]], 0)
            r = pool.push([0, 1, 2], rows)
            rest[0].append(r[0]), new.append(r[1]), rest[1].append(r[2])
        assert [int(r.shape[0]) for r in new] == [0] * 6 + [7 * (HOP if unit == 1 else 1)] + [HOP if unit == 1 else 1] * 5
        assert torch.equal(torch.cat(new, 0), lone(make_stream(1), cut(newcomer, unit)))
        for k, j in enumerate((0, 2)):
            whole = torch.cat([first[j]] + rest[k], 0)
            assert torch.equal(whole, lone(make_stream(1), [x[j, : 7 * unit]] + cut(x[j, 7 * unit:], unit))), f"slot {j}"


# ---- 6. reference parity through the pool ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,precision", [("full_noise_b2", None), ("full_tones_b2", None), ("full_noise_b2", "fp32_exact")])
def test_the_pool_matches_the_reference(name, precision, golden, codecs):
    z, meta = golden
    codec = codec_for(name, golden, codecs, precision)
    tag = f"{name}/sessions" + (f"/{precision}" if precision else "")
    F = ENCODE_FRAMES[name]
    sig = signal_of(name, GOLDEN_DIR).cuda()
    out, _ = run_staggered(codec.encode_sessions(2), [0, 3], [cut(sig[j], HOP) for j in range(2)])
    toks = torch.stack([torch.cat(o, 0) for o in out], 0)
    check_tokens(tag, toks, z[f"{name}.toks"][:, :F], z[f"{name}.margin64"][:, :F])
    gt = tokens_of(name, z, GOLDEN_DIR).cuda()
    out, _ = run_staggered(codec.decode_sessions(2), [0, 3], [cut(gt[j], 1) for j in range(2)])
    rec = torch.stack([torch.cat(o, 0) for o in out], 0).cpu().numpy()
    assert list(rec.shape) == meta["cases"][name]["rec_shape"]
    err = rms(rec.reshape(-1)[::REC_STRIDE] - z[f"{name}.rec_strided"])
    parity_record.record("encodec_dsessions", tag, waveform_rms_err=err)
    print(f"encodec_dsessions {tag}: waveform RMS error {err:.3e} (bar {WAVE_BAR:g})")
    assert err < WAVE_BAR, err


# ---- 7. ABI refusals leave everything usable ------------------------------------------------------------------------------------------
def test_abi_refusals_leave_everything_usable(codecs, mimi_checkpoints):
    import ctypes as C

    from audiocodecs_amd import Mimi
    from audiocodecs_amd.encodec import _ptr, _stream

    codec = codecs("tiny")
    B, F, K = 3, WARMUP, codec.num_codebooks
    toks_in, sig_in = rand_toks(713, B, 2 * F + 1), noise(714, B, (2 * F + 1) * HOP).cuda()
    dev = toks_in.device
    nat = codec._native_for(toks_in)
    L, h = nat.lib, nat.h
    db, eb = L.ac_encodec_stream_decode_state_bytes(h, B), L.ac_encodec_stream_state_bytes(h, B)
    dws, ews = L.ac_encodec_stream_decode_workspace_bytes(h, B, F), L.ac_encodec_stream_workspace_bytes(h, B, F)
    big = max(db, eb)
    dstate = torch.empty(big, dtype=torch.uint8, device=dev)
    estate = torch.empty(big, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(dws, ews), dtype=torch.uint8, device=dev)

    def lists(slots):
        return (C.c_int * max(len(slots), 1))(*slots), torch.tensor(slots if slots else [0], dtype=torch.int32, device=dev)

    def call(kind, slots, f=F, st=None, sb=None, wb=None, hh=h, first=0, n=None):
        """One slot push of `f` frames starting at frame `first` of the inputs; returns (rc, output)."""
        host, d = lists(slots)
        n = len(slots) if n is None else n
        rows = max(len(slots), 1)
        if kind == "dec":
            src = toks_in[:rows, first:first + f].contiguous()
            dst = torch.empty(rows, f * HOP, dtype=torch.float32, device=dev)
            rc = L.ac_encodec_stream_decode_slots(hh, _ptr(dstate if st is None else st), db if sb is None else sb, B, host, _ptr(d), n, _ptr(src), f, K,
                                                  _ptr(dst), _ptr(ws), dws if wb is None else wb, _stream())
        else:
            src = sig_in[:rows, first * HOP:(first + f) * HOP].contiguous()
            dst = torch.empty(rows, f, K, dtype=torch.int64, device=dev)
            rc = L.ac_encodec_stream_encode_slots(hh, _ptr(estate if st is None else st), eb if sb is None else sb, B, host, _ptr(d), n, _ptr(src), f, K,
                                                  _ptr(dst), _ptr(ws), ews if wb is None else wb, _stream())
        return rc, dst

    def reset_slots(kind, slots, st=None, n=None, hh=h):
        host, d = lists(slots)
        fn = L.ac_encodec_stream_decode_reset_slots if kind == "dec" else L.ac_encodec_stream_reset_slots
        state, sb = (dstate, db) if kind == "dec" else (estate, eb)
        return fn(hh, _ptr(state if st is None else st), sb, B, host, _ptr(d), len(slots) if n is None else n, _stream())

    for kind in ("dec", "enc"):
        assert call(kind, [0, 2])[0] == AC_EINVAL and reset_slots(kind, [0]) == AC_EINVAL          # never reset whole
    assert L.ac_encodec_stream_decode_reset(h, _ptr(dstate), db, B, None, _stream()) == 0
    assert L.ac_encodec_stream_reset(h, _ptr(estate), eb, B, None, _stream()) == 0
    mcfg, msd = mimi_checkpoints("tiny", 0)
    mnat = Mimi(24000, state_dict=msd, config=mcfg)._native_for(toks_in)
    for kind, own, other in (("dec", dstate, estate), ("enc", estate, dstate)):
        assert call(kind, [])[0] == AC_EINVAL and reset_slots(kind, []) == AC_EINVAL                # n = 0
        assert call(kind, [0, 1, 2], n=4)[0] == AC_EINVAL and reset_slots(kind, [0, 1, 2], n=4) == AC_EINVAL   # n > B
        for bad in ([0, B], [-1, 1]):                                                                  # a slot outside [0, B)
            assert call(kind, bad)[0] == AC_EINVAL and reset_slots(kind, bad) == AC_EINVAL
        assert call(kind, [2, 2])[0] == AC_EINVAL and reset_slots(kind, [1, 1]) == AC_EINVAL        # a repeated slot
        assert call(kind, [0, 2], f=WARMUP - 1)[0] == AC_EINVAL                                     # a fresh slot needs the warm-up
        assert call(kind, [0, 2], st=other, sb=big)[0] == AC_EINVAL                                 # the other kind of state
        assert reset_slots(kind, [0], st=other) == AC_EINVAL
        assert call(kind, [0, 2], sb=(db if kind == "dec" else eb) - 256)[0] == AC_ENOMEM           # state too short
        assert call(kind, [0, 2], wb=4096)[0] == AC_ENOMEM                                          # workspace too short
        assert call(kind, [0, 2], hh=mnat.h)[0] == AC_EINVAL and reset_slots(kind, [0], hh=mnat.h) == AC_EINVAL   # a Mimi handle
    # after all of them: the bits of a pool that was never refused anything
    pd, pe = codec.decode_sessions(B), codec.encode_sessions(B)
    for p in (pd, pe):
        [p.open() for _ in range(B)]
    for kind, pool, x, unit in (("dec", pd, toks_in, 1), ("enc", pe, sig_in, HOP)):
        rc, got = call(kind, [2, 0])
        assert rc == 0
        want = pool.push([2, 0], x[:2, : F * unit].contiguous())
        assert torch.equal(got, torch.stack(want, 0))
        assert call(kind, [2, 0], f=1, first=F)[0] == 0                                             # F = 1 once warm ...
        pool.push([2, 0], x[:2, F * unit:(F + 1) * unit].contiguous())
        assert call(kind, [1, 0], f=1, first=F + 1)[0] == AC_EINVAL                                 # ... but not beside a fresh slot
        # lockstep pushes on the same state: F = 1 is refused while slot 1 is fresh, the warm-up F runs fresh and warm slots together
        if kind == "dec":
            src1, dst1 = x[:, F + 1:F + 2].contiguous(), torch.empty(B, HOP, dtype=torch.float32, device=dev)
            src7, dst7 = x[:, F + 1:].contiguous(), torch.empty(B, F * HOP, dtype=torch.float32, device=dev)
            lock = lambda s, d, f: L.ac_encodec_stream_decode(h, _ptr(dstate), db, _ptr(s), B, f, K, _ptr(d), _ptr(ws), dws, _stream())   # noqa: E731
        else:
            src1, dst1 = x[:, (F + 1) * HOP:(F + 2) * HOP].contiguous(), torch.empty(B, 1, K, dtype=torch.int64, device=dev)
            src7, dst7 = x[:, (F + 1) * HOP:].contiguous(), torch.empty(B, F, K, dtype=torch.int64, device=dev)
            lock = lambda s, d, f: L.ac_encodec_stream_encode(h, _ptr(estate), eb, _ptr(s), B, f, K, _ptr(d), _ptr(ws), ews, _stream())   # noqa: E731
        assert lock(src1, dst1, 1) == AC_EINVAL
        assert lock(src7, dst7, F) == 0
        want = pool.push([0, 1, 2], src7)
        assert torch.equal(dst7, torch.stack(want, 0))
        assert lock(src1, dst1, 1) == 0                                                              # every slot is warm now
        assert reset_slots(kind, [1]) == 0
        assert lock(src1, dst1, 1) == AC_EINVAL                                                      # and slot 1 is fresh again
    torch.cuda.synchronize()


# ---- 8. Python refusals ---------------------------------------------------------------------------------------------------------------
def test_python_refusals_leave_the_pool_as_it_was(codecs, checkpoints):
    from audiocodecs_amd import Encodec, EncodecDecodeSessions, EncodecEncodeSessions

    cfg, sd = checkpoints("tiny", 0)
    for fn in ("encode_sessions", "decode_sessions"):
        with pytest.raises(ValueError, match="resampling"):
            getattr(Encodec(16000, state_dict=sd, config=cfg), fn)(2)
    with pytest.raises(ValueError, match="decode"):
        Encodec(24000, mode="decode", state_dict=sd, config=cfg).encode_sessions(1)
    with pytest.raises(ValueError, match="encode"):
        Encodec(24000, mode="encode", state_dict=sd, config=cfg).decode_sessions(1)
    codec = codecs("tiny")
    for bad in (0, -2, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            codec.encode_sessions(bad)
        with pytest.raises(ValueError):
            codec.decode_sessions(bad)
    sig, toks = noise(715, 2, 9 * HOP).cuda(), rand_toks(716, 2, 9)
    for make_pool, cls, x, unit, bads in (
            (codec.encode_sessions, EncodecEncodeSessions, sig, HOP, lambda x: (x.double(), x.long(), x.cpu(), x[0], x[:, None])),
            (codec.decode_sessions, EncodecDecodeSessions, toks, 1, lambda x: (x.int(), x.float(), x.cpu(), x[0], x[:, :, :4]))):
        pool, clean = make_pool(3), make_pool(3)
        assert isinstance(pool, cls)
        for p in (pool, clean):
            assert [p.open(), p.open(), p.open()] == [0, 1, 2]
            p.close(1)
        with pytest.raises(ValueError):
            pool.push([0, 1], x)                         # a closed slot
        with pytest.raises(ValueError):
            pool.close(1)
        with pytest.raises(ValueError):
            pool.push([0, 3], x)                         # out of range
        with pytest.raises(ValueError):
            pool.push([0, 0], x)                         # repeated
        with pytest.raises(ValueError):
            pool.push([0], x)                            # wrong row count
        with pytest.raises(ValueError):
            pool.push([0, 2, 1], x)
        with pytest.raises(ValueError):
            pool.pending(1)
        for bad in bads(x):
            with pytest.raises(ValueError):
                pool.push([0, 2], bad)
        assert pool.open() == 1
        with pytest.raises(ValueError):
            pool.open()                                  # full
        pool.close(1)
        assert pool.active == clean.active == [0, 2]
        for cutp in (x[:, : 3 * unit], x[:, 3 * unit: 8 * unit], x[:, 8 * unit:]):
            got, want = pool.push([0, 2], cutp.contiguous()), clean.push([0, 2], cutp.contiguous())
            for g, w in zip(got, want):
                assert torch.equal(g, w)
        assert pool.frames(0) == clean.frames(0) == 9
