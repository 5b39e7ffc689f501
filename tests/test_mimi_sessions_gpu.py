"""Session pools on Mimi streams (Mimi.encode_sessions / decode_sessions, include/audiocodecs_amd.h ac_mimi_stream_*_slots).

A pool runs any subset of the slots of one stream state, every slot at its own transformer position.  The contract is bitwise:
n listed slots give the bits of the lockstep stream of batch n fed the same rows -- whichever slots they sit in, in whatever order
they are listed, whatever the unlisted slots hold -- and a session gives the bits of a lone `encode_stream(1)` / `decode_stream(1)`
fed the same pieces (on the decode side: while both take the same linear route, which the tests force).
MIMI_TINY (window 6, ring of 5 rows, 2 positions per frame) wraps its ring after 3 frames; the full configuration appears where
head_dim 64 and the window of 250 matter.  The lockstep streams' own parity with the reference is tests/test_mimi_stream_gpu.py and
tests/test_mimi_dstream_gpu.py; case 7 here runs the reference's fixtures through the pools all the same."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from golden_cases import noise
from mimi_cases import REC_STRIDE
from mimi_dstream_cases import case_of as dcase_of, schedule, tokens_of
from mimi_stream_cases import CASES, HOP, make_signal
from test_mimi_dstream_gpu import AC_EINVAL, AC_ENOMEM, BAR, codecs, rand_toks, set_route  # noqa: F401 (codecs: fixture)
from test_mimi_stream_gpu import check_tokens, stream_golden  # noqa: F401 (stream_golden: fixture)
from test_gpu_parity import rms
import parity_record

pytestmark = pytest.mark.gpu

ROUTES = [0, 1]      # ac_debug_set "mstream_skinny": the decode stream's linear layers through the tap-GEMM / mstream_linear_kernel


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def route(request, codecs):
    """Force the decode route on both configurations for one test; auto (-1) again afterwards."""
    used = [codecs("tiny"), codecs("full")]
    for c in used:
        set_route(c, request.param)
    yield request.param
    for c in used:
        set_route(c, -1)


def sides(codec, seed, rows, frames):
    """(make_pool, make_stream, x [rows, frames * unit], unit) for the encode side and the decode side."""
    return ((codec.encode_sessions, codec.encode_stream, noise(seed, rows, frames * HOP).cuda(), HOP),
            (codec.decode_sessions, codec.decode_stream, rand_toks(seed + 1, rows, frames), 1))


def side(codec, kind, seed, rows, frames):
    return sides(codec, seed, rows, frames)[0 if kind == "encode" else 1]


def cuts(x, sizes, unit):
    """x [n, T, ...] -> pushes of `sizes` frames (the whole of x)."""
    out, t = [], 0
    for f in sizes:
        out.append(x[:, t * unit:(t + f) * unit].contiguous())
        t += f
    assert t * unit == x.shape[1]
    return out


def feed(pool, slots, pushes):
    """Push a list of [n, ...] tensors to the same slots; per slot the concatenated result."""
    acc = [[] for _ in slots]
    for x in pushes:
        res = pool.push(slots, x)
        assert len(res) == len(slots)
        for i, r in enumerate(res):
            acc[i].append(r)
    return [torch.cat(a, 0) for a in acc]


def lockstep(stream, pushes):
    """The concatenated output [n, ...] of a lockstep stream fed `pushes`."""
    return torch.cat([stream.push(p) for p in pushes], 1)


def lone(stream, pieces):
    """The concatenated output of a batch-1 lockstep stream fed one session's pieces ([L] samples or [F, K] tokens each)."""
    return torch.cat([stream.push(p[None]) for p in pieces], 1)[0]


def open_all(pool):
    got = [pool.open() for _ in range(pool.capacity)]
    assert got == list(range(pool.capacity)) and pool.active == got
    return got


# ---- 1. a listed subset is the lockstep stream of its size -----------------------------------------------------------------------------
SUBSET = [("tiny", 5, [4, 2, 0], [1] * 8), ("tiny", 5, [4, 2, 0], [3, 3, 2]), ("tiny", 5, [4, 2, 0], [1, 2, 5]), ("full", 4, [3, 1, 0], [1, 2, 1])]
SUBSET_IDS = ["tiny-ones", "tiny-overwrite", "tiny-ragged", "full"]


def subset_is_lockstep(codec, kind, cap, slots, sizes):
    """Descending slots: the map is nowhere the identity.  F = 3 on MIMI_TINY brings 6 rows to a ring of 5 (the append overwrites rows
    the push's own queries read: the ring-overwrite rule); [1, 2, 5] crosses a wrap inside a push."""
    make_pool, make_stream, x, unit = side(codec, kind, 801, len(slots), sum(sizes))
    pool = make_pool(cap)
    open_all(pool)
    pushes = cuts(x, sizes, unit)
    got = feed(pool, slots, pushes)
    want = lockstep(make_stream(len(slots)), pushes)
    for i, s in enumerate(slots):
        assert got[i].dtype == want.dtype and got[i].shape == want[i].shape
        assert torch.equal(got[i], want[i]), f"row {i} (slot {s})"
        assert pool.frames(s) == sum(sizes) and pool.pending(s) == 0


@pytest.mark.parametrize("cfg,cap,slots,sizes", SUBSET, ids=SUBSET_IDS)
def test_a_listed_encode_subset_is_the_lockstep_stream_of_its_size(cfg, cap, slots, sizes, codecs):
    subset_is_lockstep(codecs(cfg), "encode", cap, slots, sizes)


@pytest.mark.parametrize("route", ROUTES, indirect=True)
@pytest.mark.parametrize("cfg,cap,slots,sizes", SUBSET, ids=SUBSET_IDS)
def test_a_listed_decode_subset_is_the_lockstep_stream_of_its_size(cfg, cap, slots, sizes, route, codecs):
    subset_is_lockstep(codecs(cfg), "decode", cap, slots, sizes)


# ---- 2. staggered sessions are the lone streams ------------------------------------------------------------------------------------------
def test_staggered_encode_sessions_are_the_lone_streams(codecs):
    """A runs 7 frames alone (and is left half a frame pending), then B opens: A at position 14 -- its ring of 5 has wrapped twice --
    and B at 0 share every launch.  The tick of 1.5 frames completes two frames of A and one of B: two groups, two native calls."""
    codec = codecs("tiny")
    half = HOP // 2
    a_alone = [HOP] * 6 + [HOP + half]
    joint = [HOP, HOP, HOP + half, HOP, HOP]                 # per tick, the same count for both rows
    b_alone = [HOP] * 4
    xa = noise(811, 1, sum(a_alone) + sum(joint))[0].cuda()
    xb = noise(812, 1, sum(joint) + sum(b_alone))[0].cuda()
    pa = list(torch.split(xa, a_alone + joint))
    pb = list(torch.split(xb, joint + b_alone))
    pool = codec.encode_sessions(3)
    a = pool.open()
    out_a = [pool.push([a], p[None])[0] for p in pa[:7]]
    assert pool.frames(a) == 7 and pool.pending(a) == half
    b = pool.open()
    assert (a, b) == (0, 1) and pool.frames(b) == 0
    out_b = []
    for t in range(len(joint)):
        ra, rb = pool.push([a, b], torch.stack([pa[7 + t], pb[t]], 0))
        out_a.append(ra), out_b.append(rb)
    assert [int(r.shape[0]) for r in out_a[7:]] == [1, 1, 2, 1, 1] and [int(r.shape[0]) for r in out_b] == [1] * 5
    assert pool.frames(a) == 13 and pool.pending(a) == 0 and pool.frames(b) == 5 and pool.pending(b) == half
    pool.close(a)
    assert pool.active == [b]
    out_b += [pool.push([b], p[None])[0] for p in pb[5:]]
    assert torch.equal(torch.cat(out_a, 0), lone(codec.encode_stream(1), pa))
    assert torch.equal(torch.cat(out_b, 0), lone(codec.encode_stream(1), pb))
    assert pool.frames(b) == 9


@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_staggered_decode_sessions_are_the_lone_streams(route, codecs):
    """The decode side of the test above.  A decode push gives every listed row the same frame count, so the tick in which A brings
    two frames and B one is two pushes (two native calls all the same)."""
    codec = codecs("tiny")
    a_frames = [1] * 7 + [1, 1, 2, 1, 1]
    b_frames = [1] * 5 + [1] * 4
    ta, tb = rand_toks(813, 1, sum(a_frames))[0], rand_toks(814, 1, sum(b_frames))[0]
    pa, pb = list(torch.split(ta, a_frames)), list(torch.split(tb, b_frames))
    pool = codec.decode_sessions(3)
    a = pool.open()
    out_a = [pool.push([a], p[None])[0] for p in pa[:7]]
    b = pool.open()
    out_b = []
    for t in range(5):
        if pa[7 + t].shape[0] == pb[t].shape[0]:
            ra, rb = pool.push([a, b], torch.stack([pa[7 + t], pb[t]], 0))
        else:
            (rb,), (ra,) = pool.push([b], pb[t][None]), pool.push([a], pa[7 + t][None])
        out_a.append(ra), out_b.append(rb)
    assert pool.frames(a) == 13 and pool.frames(b) == 5
    pool.close(a)
    out_b += [pool.push([b], p[None])[0] for p in pb[5:]]
    assert torch.equal(torch.cat(out_a, 0), lone(codec.decode_stream(1), pa))
    assert torch.equal(torch.cat(out_b, 0), lone(codec.decode_stream(1), pb))


# ---- 3. the same on the full configuration, across the real window -----------------------------------------------------------------------
def across_the_window(codec, kind):
    """130 frames = 260 positions > 249: the old slot's ring has wrapped when the fresh slot joins it."""
    make_pool, make_stream, x, unit = side(codec, kind, 821, 2, 133)
    old = list(torch.split(x[0], [25 * unit] * 5 + [5 * unit] + [unit] * 3))
    new = list(torch.split(x[1, : 3 * unit], unit))
    pool = make_pool(2)
    a = pool.open()
    out_a = [pool.push([a], p[None])[0] for p in old[:6]]
    assert pool.frames(a) == 130 and codec.config.resample_stride * 130 > codec.config.sliding_window - 1
    b = pool.open()
    out_b = []
    for t in range(3):
        rb, ra = pool.push([b, a], torch.stack([new[t], old[6 + t]], 0))
        out_a.append(ra), out_b.append(rb)
    assert torch.equal(torch.cat(out_a, 0), lone(make_stream(1), old))
    assert torch.equal(torch.cat(out_b, 0), lone(make_stream(1), new))


def test_a_wrapped_and_a_fresh_encode_session_share_a_push(codecs):
    across_the_window(codecs("full"), "encode")


@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_a_wrapped_and_a_fresh_decode_session_share_a_push(route, codecs):
    across_the_window(codecs("full"), "decode")


# ---- 4. order and neighbours do not matter -----------------------------------------------------------------------------------------------
def order_and_neighbours(codec, kind):
    sizes = [1, 2, 3, 1, 1]
    make_pool, make_stream, x, unit = side(codec, kind, 831, 3, sum(sizes))
    spoiled = x.clone()
    if kind == "encode":
        spoiled[2] = float("nan")                              # the third slot's samples
    else:
        spoiled[2] = rand_toks(833, 1, sum(sizes))[0]          # (tokens have no NaN: other tokens)
    want = [lone(make_stream(1), [p[0] for p in cuts(x[j:j + 1], sizes, unit)]) for j in range(2)]
    for sa, sb in ((0, 1), (3, 1)):
        for flip in (False, True):
            for rows in (x, spoiled):
                pool = make_pool(4)
                open_all(pool)
                listed, order = ([sb, 2, sa], [1, 2, 0]) if flip else ([sa, 2, sb], [0, 2, 1])
                got = feed(pool, listed, cuts(rows[order], sizes, unit))
                res = dict(zip(listed, got))
                assert torch.equal(res[sa], want[0]) and torch.equal(res[sb], want[1]), (sa, sb, flip)


def test_order_and_neighbours_do_not_matter_to_encode_sessions(codecs):
    order_and_neighbours(codecs("tiny"), "encode")


@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_order_and_neighbours_do_not_matter_to_decode_sessions(route, codecs):
    order_and_neighbours(codecs("tiny"), "decode")


# ---- 5. unlisted slots are untouched -----------------------------------------------------------------------------------------------------
def state_sections(cfg, kind, B):
    """[(name, offset, bytes per slot)] of a Mimi stream state of B slots, and its size: the layout of DESIGN.md sections 8b / 8c
    (every section 256-byte aligned behind a 256-byte header; every section is [B]-leading)."""
    up = lambda n: -(-n // 256) * 256      # noqa: E731
    off, out = 256, []

    def take(name, per_slot):
        nonlocal off
        out.append((name, off, per_slot))
        off += up(B * per_slot)

    take("position", 8)
    take("fresh", 4)
    nr, D = len(cfg.upsampling_ratios), cfg.seanet_dim
    if kind == "encode":      # stem, (block k3, down-sampler) per ratio, final conv, down-sampler
        take("stem", (cfg.kernel_size - 1) * 4)
        ch = cfg.num_filters
        for i in range(nr):
            take(f"block{i}", (cfg.residual_kernel_size - 1) * ch * 4)
            take(f"down{i}", cfg.upsampling_ratios[nr - 1 - i] * ch * 4)
            ch *= 2
        take("final", (cfg.last_kernel_size - 1) * ch * 4)
        take("resample", cfg.resample_stride * cfg.hidden_size * 4)
    else:                     # up-sampler input, first conv, (transposed conv input, block k3) per ratio, head conv
        take("upsample", cfg.hidden_size * 4)
        take("first", (cfg.kernel_size - 1) * cfg.hidden_size * 4)
        ch = D
        for i in range(nr):
            take(f"up{i}", ch * 4)
            ch //= 2
            take(f"block{i}", (cfg.residual_kernel_size - 1) * ch * 4)
        take("head", (cfg.last_kernel_size - 1) * ch * 4)
    ring = (cfg.sliding_window - 1) * cfg.num_attention_heads * cfg.head_dim * 4
    for l in range(cfg.num_hidden_layers):
        take(f"keys{l}", ring)
        take(f"values{l}", ring)
    return out, off


def unlisted_untouched(codec, kind):
    cap, listed = 4, [3, 1]
    make_pool, make_stream, x, unit = side(codec, kind, 841, cap, 9)
    pool = make_pool(cap)
    secs, total = state_sections(codec.config, kind, cap)
    assert total == pool._state.numel(), "the test's layout is not the library's"
    open_all(pool)
    pool.push([0, 1, 2, 3], x[:, : 2 * unit].contiguous())              # every slot holds something
    pool.push([2, 3], x[2:4, 2 * unit: 3 * unit].contiguous())          # ... at positions of their own
    torch.cuda.synchronize()
    for first, f in ((3, 3), (6, 1)):                                   # F = 3: six rows into the ring of five; F = 1: the short-chunk staging
        before = pool._state.cpu().numpy().copy()
        pool.push(listed, x[listed, first * unit:(first + f) * unit].contiguous())
        torch.cuda.synchronize()
        after = pool._state.cpu().numpy()
        owned = np.zeros(total, dtype=bool)                              # bytes of the listed slots' sections
        for name, off, per in secs:
            for s in listed:
                owned[off + s * per: off + (s + 1) * per] = True
            for s in listed:
                assert (before[off + s * per: off + (s + 1) * per] != after[off + s * per: off + (s + 1) * per]).any() or name == "fresh", (name, s)
        stray = np.nonzero((before != after) & ~owned)[0]
        assert stray.size == 0, f"{stray.size} bytes outside the listed slots changed, the first at {int(stray[0])}"
    # and behaviourally: slot 0 sat out both pushes and goes on as its lone stream does
    got = pool.push([0], x[0:1, 2 * unit:].contiguous())[0]
    s = make_stream(1)
    s.push(x[0:1, : 2 * unit].contiguous())
    assert torch.equal(got, s.push(x[0:1, 2 * unit:].contiguous())[0])


def test_unlisted_encode_slots_are_untouched(codecs):
    unlisted_untouched(codecs("tiny"), "encode")


@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_unlisted_decode_slots_are_untouched(route, codecs):
    unlisted_untouched(codecs("tiny"), "decode")


# ---- 6. a reused slot starts from nothing ------------------------------------------------------------------------------------------------
def reused_slot(codec, kind):
    """The reset does not clear the rings: what the first session left in them is masked by the position rule alone."""
    sizes = [1, 3, 5]
    make_pool, make_stream, x, unit = side(codec, kind, 851, 2, 18)
    first, second = x[1:2, : 9 * unit], x[1:2, 9 * unit:]
    other = cuts(x[0:1], sizes + sizes, unit)
    pool = make_pool(2)
    open_all(pool)
    got_other = []
    for p, q in zip(cuts(first, sizes, unit), other[:3]):
        got_other.append(pool.push([1, 0], torch.cat([p, q], 0))[1])
    assert pool.frames(1) == 9
    pool.close(1)
    assert pool.active == [0] and pool.open() == 1 and pool.frames(1) == 0 and pool.pending(1) == 0
    got = []
    for p, q in zip(cuts(second, sizes, unit), other[3:]):
        r = pool.push([1, 0], torch.cat([p, q], 0))
        got.append(r[0]), got_other.append(r[1])
    got = torch.cat(got, 0)
    assert torch.equal(got, lockstep(make_stream(1), cuts(second, sizes, unit))[0])
    cont = make_stream(1)
    lockstep(cont, cuts(first, sizes, unit))
    assert not torch.equal(got, lockstep(cont, cuts(second, sizes, unit))[0])        # the continuation is something else
    assert torch.equal(torch.cat(got_other, 0), lockstep(make_stream(1), other)[0])   # and the neighbour never noticed


def test_a_reused_encode_slot_starts_from_nothing(codecs):
    reused_slot(codecs("tiny"), "encode")


@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_a_reused_decode_slot_starts_from_nothing(route, codecs):
    reused_slot(codecs("tiny"), "decode")


# ---- 7. reference parity through the pools -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_the_encode_pool_matches_the_reference(case, stream_golden, codecs):
    z, meta = stream_golden
    name = case["name"]
    info = meta["cases"][name]
    codec = codecs(case["cfg"], case["weights_seed"])
    sig = torch.from_numpy(make_signal(case, GOLDEN_DIR)).cuda()
    rows = info["B"]
    pool = codec.encode_sessions(rows + 1)
    open_all(pool)
    pool.close(0)
    slots = list(range(rows, 0, -1))                          # row i is the session in slot rows - i
    toks = torch.stack(feed(pool, slots, cuts(sig, info["pushes"], HOP)), 0)
    gold, margin = z[f"{name}_stream"], z[f"{name}_margin"]
    mism = int((toks.cpu().numpy() != gold.astype(np.int64)).sum())
    parity_record.record("mimi_sessions", name, tokens_compared=int(gold.size), tokens_differing=mism)
    print(f"mimi_sessions {name}: {mism} of {gold.size} tokens differ from the fixture's")
    check_tokens(toks, gold, margin)                          # zero mismatches outside fp64 near-ties, as for the lockstep stream


@pytest.mark.parametrize("name", ["tiny_taps", "tiny_odd", "full_noise_b2"])
def test_the_decode_pool_matches_the_reference(name, mimi_golden, codecs):
    z, meta = mimi_golden
    case = dcase_of(name)
    codec = codecs(case["cfg"], case["weights_seed"], meta["cases"][name]["K"])
    set_route(codec, -1)
    toks = tokens_of(name, z, GOLDEN_DIR).cuda()
    rows = toks.shape[0]
    pool = codec.decode_sessions(rows + 1)
    open_all(pool)
    pool.close(0)
    slots = list(range(rows, 0, -1))
    rec = torch.stack(feed(pool, slots, cuts(toks, schedule("ragged", toks.shape[1]), 1)), 0).cpu().numpy()
    assert list(rec.shape) == meta["cases"][name]["rec_shape"]
    err = rms(rec.reshape(-1)[::REC_STRIDE] - z[f"{name}.rec_strided"])
    parity_record.record("mimi_dsessions", f"{name}/ragged", waveform_rms_err=err)
    print(f"mimi_dsessions {name}/ragged: waveform RMS error {err:.3e} (bar {BAR:g})")
    assert err < BAR, err


# ---- 8. graph capture --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, indirect=True)
def test_a_captured_slot_push_replays_on_new_tokens_and_slots(route, codecs):
    """The slot list, like position and `fresh`, is read on the device: one captured n = 2, F = 1 slot push, replayed after its token
    buffer AND its device slot list were overwritten, is the eager call on those slots -- output and state, bit for bit."""
    from audiocodecs_amd.encodec import _ptr, _stream

    codec = codecs("full")
    cap, n, F, K = 4, 2, 1, codec.num_codebooks
    hop = codec.config.hop_length
    toks = rand_toks(861, cap, 6)
    nat = codec._native_for(toks)
    L, h, dev = nat.lib, nat.h, toks.device
    sb = L.ac_mimi_stream_decode_state_bytes(h, cap)
    wsb = max(L.ac_mimi_stream_decode_workspace_bytes(h, cap, F), L.ac_mimi_stream_decode_workspace_bytes(h, n, F))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    states = [torch.zeros(sb, dtype=torch.uint8, device=dev) for _ in range(2)]      # [0]: replayed, [1]: eager
    sig = [torch.zeros(n, F * hop, dtype=torch.float32, device=dev) for _ in range(2)]
    all_sig = torch.empty(cap, F * hop, dtype=torch.float32, device=dev)
    tx = torch.empty(n, F, K, dtype=torch.int64, device=dev)
    sx = torch.empty(n, dtype=torch.int32, device=dev)

    def slot_push(i, host_slots):
        host = (C.c_int * n)(*host_slots)
        return L.ac_mimi_stream_decode_slots(h, _ptr(states[i]), sb, cap, host, _ptr(sx), n, _ptr(tx), F, K, _ptr(sig[i]), _ptr(ws), wsb, _stream())

    def load(slots, frame):
        sx.copy_(torch.tensor(slots, dtype=torch.int32))
        tx.copy_(toks[slots, frame:frame + F])

    for i in range(2):       # both states alike: every slot one frame in, then slots 0 and 1 one more (the slot call's buffers exist)
        assert L.ac_mimi_stream_decode_reset(h, _ptr(states[i]), sb, cap, None, _stream()) == 0
        src = toks[:, :1].contiguous()
        assert L.ac_mimi_stream_decode(h, _ptr(states[i]), sb, _ptr(src), cap, F, K, _ptr(all_sig), _ptr(ws), wsb, _stream()) == 0
        load([0, 1], 1)
        assert slot_push(i, [0, 1]) == 0
        torch.cuda.synchronize()
    assert torch.equal(states[0], states[1])
    g = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(g, stream=stream):
            assert slot_push(0, [0, 1]) == 0                 # (the host list serves the checks of this call only)
    for slots, frame in (([0, 1], 2), ([3, 2], 1), ([2, 0], 2)):
        load(slots, frame)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert slot_push(1, slots) == 0
        torch.cuda.synchronize()
        assert torch.equal(sig[0], sig[1]), slots
        assert torch.equal(states[0], states[1]), slots
    assert not torch.isnan(sig[0]).any() and float(sig[0].abs().max()) > 0


# ---- 9. ABI refusals leave everything usable ----------------------------------------------------------------------------------------------
def test_abi_refusals_leave_everything_usable(codecs, checkpoints):
    from audiocodecs_amd import Encodec
    from audiocodecs_amd.encodec import _ptr, _stream

    codec = codecs("tiny")
    B, F, K = 3, 2, codec.num_codebooks
    toks_in, sig_in = rand_toks(871, B, 2 * F), noise(872, B, 2 * F * HOP).cuda()
    dev = toks_in.device
    nat = codec._native_for(toks_in)
    L, h = nat.lib, nat.h
    db, eb = L.ac_mimi_stream_decode_state_bytes(h, B), L.ac_mimi_stream_state_bytes(h, B)
    dws, ews = L.ac_mimi_stream_decode_workspace_bytes(h, 2, F), L.ac_mimi_stream_workspace_bytes(h, 2, F)
    assert min(db, eb, dws, ews) > 0
    big = max(db, eb)
    dstate = torch.zeros(big, dtype=torch.uint8, device=dev)
    estate = torch.zeros(big, dtype=torch.uint8, device=dev)
    never = torch.zeros(big, dtype=torch.uint8, device=dev)
    ws = torch.empty(max(L.ac_mimi_stream_decode_workspace_bytes(h, B, F), L.ac_mimi_stream_workspace_bytes(h, B, F)), dtype=torch.uint8, device=dev)

    def call(kind, slots, st=None, sb=None, wb=None, hh=h, first=0, n=None, cap=B, null=()):
        """One slot push of F frames starting at frame `first` of the inputs; returns (rc, output)."""
        host = (C.c_int * max(len(slots), 1))(*slots)
        d = torch.tensor(slots if slots else [0], dtype=torch.int32, device=dev)
        n = len(slots) if n is None else n
        rows = max(len(slots), 1)
        host_arg, dev_arg = (None if "host" in null else host), (None if "dev" in null else _ptr(d))
        if kind == "dec":
            src = toks_in[:rows, first:first + F].contiguous()
            dst = torch.empty(rows, F * HOP, dtype=torch.float32, device=dev)
            rc = L.ac_mimi_stream_decode_slots(hh, _ptr(dstate if st is None else st), db if sb is None else sb, cap, host_arg, dev_arg, n, _ptr(src), F, K,
                                               _ptr(dst), _ptr(ws), dws if wb is None else wb, _stream())
        else:
            src = sig_in[:rows, first * HOP:(first + F) * HOP].contiguous()
            dst = torch.empty(rows, F, K, dtype=torch.int64, device=dev)
            rc = L.ac_mimi_stream_encode_slots(hh, _ptr(estate if st is None else st), eb if sb is None else sb, cap, host_arg, dev_arg, n, _ptr(src), F, K,
                                               _ptr(dst), _ptr(ws), ews if wb is None else wb, _stream())
        return rc, dst

    for kind in ("dec", "enc"):
        assert call(kind, [0, 2])[0] == AC_EINVAL                                                 # never reset
    assert L.ac_mimi_stream_decode_reset(h, _ptr(dstate), db, B, None, _stream()) == 0
    assert L.ac_mimi_stream_reset(h, _ptr(estate), eb, B, None, _stream()) == 0
    ecfg, esd = checkpoints("tiny", 0)
    enat = Encodec(24000, num_codebooks=2, state_dict=esd, config=ecfg)._native_for(toks_in)
    for kind, own, other in (("dec", dstate, estate), ("enc", estate, dstate)):
        assert call(kind, [])[0] == AC_EINVAL                                                     # n = 0
        assert call(kind, [0, 1, 2], n=4)[0] == AC_EINVAL                                         # n > B
        for bad in ([0, B], [-1, 1]):                                                             # a slot outside [0, B)
            assert call(kind, bad)[0] == AC_EINVAL
        assert call(kind, [2, 2])[0] == AC_EINVAL                                                 # a repeated slot
        assert call(kind, [0, 2], null=("host",))[0] == AC_EINVAL                                 # a null list
        assert call(kind, [0, 2], null=("dev",))[0] == AC_EINVAL
        assert call(kind, [0, 2], cap=B + 1, sb=big + (1 << 20))[0] == AC_EINVAL                  # reset for another B
        assert call(kind, [0, 1], cap=2)[0] == AC_EINVAL
        assert call(kind, [0, 2], st=other, sb=big)[0] == AC_EINVAL                               # the other kind of state
        assert call(kind, [0, 2], st=never, sb=big)[0] == AC_EINVAL                               # a state never reset
        assert call(kind, [0, 2], sb=(db if kind == "dec" else eb) - 256)[0] == AC_ENOMEM         # state too short
        assert call(kind, [0, 2], wb=(dws if kind == "dec" else ews) - 1)[0] == AC_ENOMEM         # workspace one byte short
        assert call(kind, [0, 2], hh=enat.h)[0] == AC_EINVAL                                      # an EnCodec handle
    # after all of them: the bits of a pool that was never refused anything
    pd, pe = codec.decode_sessions(B), codec.encode_sessions(B)
    for kind, pool, x, unit in (("dec", pd, toks_in, 1), ("enc", pe, sig_in, HOP)):
        open_all(pool)
        for first, slots in ((0, [2, 0]), (F, [2, 0])):
            rc, got = call(kind, slots, first=first)
            assert rc == 0
            want = pool.push(slots, x[:2, first * unit:(first + F) * unit].contiguous())
            torch.cuda.synchronize()
            assert torch.equal(got, torch.stack(want, 0)), (kind, first)
    torch.cuda.synchronize()


# ---- 10. Python refusals -----------------------------------------------------------------------------------------------------------------
def test_python_refusals_leave_the_pool_as_it_was(codecs, mimi_checkpoints):
    from audiocodecs_amd import Mimi, MimiDecodeSessions, MimiEncodeSessions

    cfg, sd = mimi_checkpoints("tiny", 0)
    for fn in ("encode_sessions", "decode_sessions"):
        with pytest.raises(ValueError, match="resampling"):
            getattr(Mimi(16000, state_dict=sd, config=cfg), fn)(2)
    with pytest.raises(ValueError, match="decode"):
        Mimi(24000, mode="decode", state_dict=sd, config=cfg).encode_sessions(1)
    with pytest.raises(ValueError, match="encode"):
        Mimi(24000, mode="encode", state_dict=sd, config=cfg).decode_sessions(1)
    codec = codecs("tiny")
    for bad in (0, -2, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            codec.encode_sessions(bad)
        with pytest.raises(ValueError):
            codec.decode_sessions(bad)
    sig, toks = noise(881, 2, 9 * HOP + 100).cuda(), rand_toks(882, 2, 9)
    for make_pool, cls, x, unit, bads in (
            (codec.encode_sessions, MimiEncodeSessions, sig, HOP, lambda x: (x.double(), x.long(), x.cpu(), x[0], x[:, None])),
            (codec.decode_sessions, MimiDecodeSessions, toks, 1, lambda x: (x.int(), x.float(), x.cpu(), x[0], x[:, :, :4]))):
        pool, clean = make_pool(3), make_pool(3)
        assert isinstance(pool, cls) and pool.capacity == 3 and pool.hop == HOP and pool.MAX_POSITIONS == 1 << 24
        for p in (pool, clean):
            assert [p.open(), p.open(), p.open()] == [0, 1, 2]
            p.close(1)
            p.push([0, 2], x[:, : 2 * unit + unit // 3].contiguous())

        def snapshot(p):
            return p.active, [p.pending(s) for s in p.active], [p.frames(s) for s in p.active]

        was = snapshot(pool)
        assert was == ([0, 2], [unit // 3] * 2, [2, 2])

        def refused(fn, *args):
            with pytest.raises(ValueError):
                fn(*args)
            assert snapshot(pool) == was

        rest = x[:, 2 * unit + unit // 3:]
        refused(pool.push, [0, 1], rest)                 # a closed slot
        refused(pool.close, 1)
        refused(pool.pending, 1)
        refused(pool.frames, 1)
        refused(pool.push, [0, 3], rest)                 # out of range
        refused(pool.push, [0, -1], rest)
        refused(pool.push, [0, True], rest)
        refused(pool.push, [0, 0], rest)                 # repeated
        refused(pool.push, [0], rest)                    # wrong row count
        refused(pool.push, [0, 2, 1], rest)
        refused(pool.push, 0, rest)                      # not a sequence
        for bad in bads(rest):
            refused(pool.push, [0, 2], bad)              # dtype, device, shape
        assert pool.open() == 1
        with pytest.raises(ValueError, match="full"):
            pool.open()
        pool.close(1)
        assert snapshot(pool) == was
        pool.MAX_POSITIONS = 2 * 5                       # on the instance: slot 0 and 2 have run 2 frames, 3 more fit, 7 do not
        refused(pool.push, [0, 2], rest)
        fresh = pool.open()                              # a session reopened in a slot counts from 0 -- and is refused by its own count
        assert fresh == 1
        refused_was = snapshot(pool)
        with pytest.raises(ValueError, match="positions"):
            pool.push([1], rest[:1])
        assert snapshot(pool) == refused_was
        ok = pool.push([1], rest[:1, : 5 * unit].contiguous())      # 5 frames from 0 fit
        assert pool.frames(1) == 5 and ok[0].shape[0] == 5 * (HOP if unit == 1 else 1)
        pool.close(1)
        del pool.MAX_POSITIONS
        assert pool.MAX_POSITIONS == 1 << 24
        for cutp in (rest[:, : 3 * unit], rest[:, 3 * unit:]):
            got, want = pool.push([0, 2], cutp.contiguous()), clean.push([0, 2], cutp.contiguous())
            for g, w in zip(got, want):
                assert torch.equal(g, w)
        assert pool.frames(0) == clean.frames(0) == 9 and snapshot(pool) == snapshot(clean)
