"""The stateful resampler on the GPU: alone (audiocodecs_amd.ResampleStream, ac_resample_stream_*) and inside the four codec streams
(`encode_stream` / `decode_stream(..., resample=True)`).

The contract is bit equality with the one-shot kernel: whatever the push schedule, the concatenated pushes and the closing `finish`
are `torch.equal` to `resample` on the whole signal (the same fp32 chain per output).  Against the fp64 oracle the bars are those of
tests/test_resample.py (2e-6 at 16 <-> 24 kHz, 3e-5 with 44.1 kHz).  Inside the codecs the resampling streams are compared bitwise
with the plain streams fed by a standalone ResampleStream, and with the one-shot calls under the criteria of the existing stream
tests (their own `check_tokens`)."""
import math

import numpy as np
import pytest
import torch

from encodec_stream_cases import HOP as E_HOP, WARMUP
from golden_cases import noise
from mimi_stream_cases import HOP as M_HOP
from oracle import resample_oracle as R
from test_encodec_stream_gpu import check_tokens as encodec_check_tokens
from test_mimi_stream_gpu import check_tokens as mimi_check_tokens

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_ENOMEM = -1, -3
RATES = [(16000, 24000), (24000, 16000), (16000, 44100), (44100, 16000)]
B, L = 3, 5003
CYCLE = (7, 0, 213, 1, 320, 2)


def cycled(cycle, total):
    out, done, i = [], 0, 0
    while done < total:
        n = min(cycle[i % len(cycle)], total - done)
        out.append(n)
        done += n
        i += 1
    return out


SCHEDULES = {"all_at_once": [L], "one_sample": [1] * 40 + [L - 40], "ragged": cycled(CYCLE, L)}

_WHOLE = {}


def whole(rates):
    """(x on the device, the one-shot kernel's result, the fp64 oracle's): computed once per rate pair and left unchanged."""
    from audiocodecs_amd.resample import resample

    if rates not in _WHOLE:
        x = noise(71, B, L, amp=0.3)
        _WHOLE[rates] = (x.cuda(), resample(x.cuda(), *rates), R.resample(x.numpy(), *rates))
    return _WHOLE[rates]


def run(stream, x, sizes, finish=True):
    """Push x [B, T] in pieces of `sizes`; checks every push's shape against `out_len` and the counters; returns the list of outputs."""
    outs, t = [], 0
    for n in sizes:
        want = stream.out_len(n)
        before = (stream.consumed, stream.emitted)
        y = stream.push(x[:, t:t + n])
        t += n
        assert y.dtype == torch.float32 and y.shape == (x.shape[0], want) and want % stream.n == 0
        assert (stream.consumed, stream.emitted) == (before[0] + n, before[1] + want)
        outs.append(y)
    if finish:
        outs.append(stream.finish())
    return outs


# ---- 1. the resampler alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SCHEDULES))
@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_pushes_are_bit_equal_to_the_one_shot_kernel(rates, kind):
    from audiocodecs_amd import ResampleStream

    x, one_shot, ref64 = whole(rates)
    s = ResampleStream(*rates, B)
    assert s.latency_samples == s.width + s.o - 1 and s.taps == 2 * s.width + s.o
    got = torch.cat(run(s, x, SCHEDULES[kind]), 1)
    assert got.shape == one_shot.shape == (B, math.ceil(s.n * L / s.o)) and s.emitted == got.shape[1]
    assert torch.equal(got, one_shot)
    err = float(np.abs(got.cpu().numpy() - ref64).max())
    print(f"resample_stream {rates} {kind}: max error against fp64 {err:.3e}")
    assert err < (2e-6 if max(rates) == 24000 else 3e-5)


@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_edge_lengths_and_empty_pushes(rates):
    from audiocodecs_amd import ResampleStream
    from audiocodecs_amd.resample import resample

    x, _, _ = whole(rates)
    s = ResampleStream(*rates, B)
    for n in (0, 1, s.width + s.o - 1, s.width + s.o):
        s.reset()
        want = resample(x[:, :n].contiguous(), *rates) if n else torch.empty(B, 0, device=x.device)    # (the one-shot of nothing is nothing)
        assert want.shape == (B, math.ceil(s.n * n / s.o))
        # finish alone: nothing was complete before it, except the first group at width + o samples
        first = s.push(x[:, :n])
        assert first.shape == (B, s.n if n == s.width + s.o else 0)
        assert torch.equal(torch.cat([first, s.finish()], 1), want)
    s.reset()
    assert s.push(x[:, :0]).shape == (B, 0) and s.consumed == 0
    mid = s.push(x[:, :100])
    assert s.push(x[:, :0]).shape == (B, 0) and s.consumed == 100          # an empty push mid-stream changes nothing
    rest = s.push(x[:, 100:200])
    assert torch.equal(torch.cat([mid, rest, s.finish()], 1), resample(x[:, :200].contiguous(), *rates))


def test_streams_are_isolated_bitwise():
    from audiocodecs_amd import ResampleStream

    rates = (16000, 24000)
    x, one_shot, _ = whole(rates)
    bad = x.clone()
    bad[1] = float("nan")
    got = torch.cat(run(ResampleStream(*rates, B), bad, SCHEDULES["ragged"]), 1)
    assert bool(torch.isnan(got[1]).all())
    for slot in (0, 2):
        alone = torch.cat(run(ResampleStream(*rates, 1), x[slot:slot + 1], SCHEDULES["ragged"]), 1)
        assert torch.equal(got[slot:slot + 1], alone) and torch.equal(alone, one_shot[slot:slot + 1])


def test_reset_replays_and_finish_closes():
    from audiocodecs_amd import ResampleStream

    rates = (24000, 16000)
    x, one_shot, _ = whole(rates)
    s = ResampleStream(*rates, B)
    run(s, x[:, :1234], cycled(CYCLE, 1234), finish=False)
    s.reset()
    assert s.consumed == s.emitted == 0
    assert torch.equal(torch.cat(run(s, x, SCHEDULES["ragged"]), 1), one_shot)       # as a fresh object
    for call in (lambda: s.push(x[:, :10]), s.finish):
        with pytest.raises(ValueError, match="finish"):
            call()
    s.reset()
    assert torch.equal(torch.cat(run(s, x, SCHEDULES["all_at_once"]), 1), one_shot)
    for wrong in (x[:2], x[0], x.double(), x.cpu(), x[:, None]):
        s.reset()
        with pytest.raises(ValueError):
            s.push(wrong)
    with pytest.raises(ValueError, match="out"):
        s.push(x[:, :500], out=torch.empty(B, 5, device=x.device))
    assert torch.equal(torch.cat(run(s, x, SCHEDULES["all_at_once"]), 1), one_shot)   # the refusals changed nothing
    # `out`: rows further apart than they are long -- the samples land behind what the caller already holds
    s.reset()
    m = s.out_len(L)
    buf = torch.full((B, 11 + m + 5), -7.0, device=x.device)
    s.push(x, out=buf[:, 11:11 + m])
    assert torch.equal(buf[:, 11:11 + m], one_shot[:, :m]) and bool((buf[:, :11] == -7).all()) and bool((buf[:, 11 + m:] == -7).all())


def test_abi_errors_leave_the_state_usable():
    import ctypes as C

    from audiocodecs_amd import _native
    from audiocodecs_amd.resample import sinc_kernel

    rates = (16000, 24000)
    x, one_shot, _ = whole(rates)
    lib = _native.lib()
    kern, n, o, width = sinc_kernel(*rates)
    kern, taps = kern.cuda(), kern.shape[1]
    nbytes = lib.ac_resample_stream_state_bytes(B, taps)
    assert nbytes >= 256 + 8 * B + 4 * B * (taps - 1) and nbytes % 256 == 0
    assert lib.ac_resample_stream_state_bytes(0, taps) == 0 and lib.ac_resample_stream_state_bytes(B, 0) == 0
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=x.device)
    off = (-buf.data_ptr()) % 256
    state = buf[off:off + nbytes]
    m = lib.ac_resample_stream_out_len(0, L, n, o, width, 0)
    y = torch.zeros(B, m, device=x.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def reset(st=state, sb=nbytes, b=B, nn=n, oo=o, tt=taps, ww=width):
        return lib.ac_resample_stream_reset(ptr(st), sb, b, nn, oo, tt, ww, stream)

    def push(st=state, sb=nbytes, b=B, ll=L, consumed=0, nn=n, oo=o, tt=taps, ww=width, xp=L, yp=m, cap=m, fin=0):
        return lib.ac_resample_stream_push(ptr(st), sb, ptr(x), xp, b, ll, consumed, ptr(kern), nn, oo, tt, ww, ptr(y), yp, cap, fin, stream)

    assert reset(sb=nbytes - 256) == AC_ENOMEM
    assert reset(tt=taps + 1) == AC_EINVAL and reset(nn=0) == AC_EINVAL and reset(b=0) == AC_EINVAL       # not a filter bank's geometry
    assert reset(st=buf[off + 4:]) == AC_EINVAL                                                          # misaligned
    assert reset() == 0
    assert push(sb=nbytes - 256) == AC_ENOMEM                       # state too short
    assert push(cap=m - 1) == AC_ENOMEM                             # output buffer too short
    assert push(tt=taps - 1) == AC_EINVAL and push(ww=width + 1) == AC_EINVAL and push(oo=0) == AC_EINVAL
    assert push(ll=-1) == AC_EINVAL and push(consumed=-1) == AC_EINVAL
    assert push(xp=L - 1) == AC_EINVAL and push(yp=m - 1) == AC_EINVAL                                     # a pitch shorter than its row
    assert push(st=buf[off + 4:]) == AC_EINVAL
    torch.cuda.synchronize()
    assert bool((y == 0).all())                                     # nothing was launched
    assert push() == 0                                              # ... and the state still works
    torch.cuda.synchronize()
    assert torch.equal(y, one_shot[:, :m])
    # what only the device can know: a count that is not the state's gives NaN, and leaves the state as it was
    tail = lib.ac_resample_stream_out_len(L, 0, n, o, width, 1)
    assert m + tail == one_shot.shape[1]
    wide = tail + n                                                 # rows `wide` apart: the short count's closing push is no longer than that
    assert lib.ac_resample_stream_out_len(L - 2, 0, n, o, width, 1) <= wide
    yt = torch.zeros(B, wide, device=x.device)
    assert lib.ac_resample_stream_push(ptr(state), nbytes, None, 0, B, 0, L - 2, ptr(kern), n, o, taps, width, ptr(yt), wide, wide, 1, stream) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(yt[:, 0]).all())
    assert lib.ac_resample_stream_push(ptr(state), nbytes, None, 0, B, 0, L, ptr(kern), n, o, taps, width, ptr(yt), wide, wide, 1, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(yt[:, :tail], one_shot[:, m:])


# ---- 2. inside the codec streams ----------------------------------------------------------------------------------------------------
FRAMES = 30
ODD = 37          # samples beyond the 30 frames: a trailing partial frame stays pending


def sizes_16k(hop, cycle):
    total = FRAMES * hop * 2 // 3 + ODD
    return total, cycled(cycle, total)


@pytest.fixture(scope="module")
def encodecs(checkpoints):
    from audiocodecs_amd import Encodec

    cfg, sd = checkpoints("tiny", 0)
    return cfg, sd, Encodec(16000, state_dict=sd, config=cfg).eval(), Encodec(24000, state_dict=sd, config=cfg).eval()


@pytest.fixture(scope="module")
def mimis(mimi_checkpoints):
    from audiocodecs_amd import Mimi

    cfg, sd = mimi_checkpoints("tiny", 0)
    return cfg, sd, Mimi(16000, state_dict=sd, config=cfg).eval(), Mimi(24000, state_dict=sd, config=cfg).eval()


def encode_both_ways(c16, c24, sig, sizes, hop, warmup):
    """The resampling stream next to the plain stream behind a standalone resampler, push for push; returns the tokens."""
    from audiocodecs_amd import ResampleStream

    s, plain, rs = c16.encode_stream(2, resample=True), c24.encode_stream(2), ResampleStream(16000, 24000, 2)
    outs, t, released = [], 0, False
    for n in sizes + [None]:
        if n is None:
            a, b = s.finish(), plain.push(rs.finish())
        else:
            a, b = s.push(sig[:, t:t + n]), plain.push(rs.push(sig[:, t:t + n]))
            t += n
        assert torch.equal(a, b) and s.pending == plain.pending
        whole_frames = rs.emitted // hop                    # frames are counted after resampling
        if not released and whole_frames < warmup:
            assert a.shape[1] == 0
        elif not released:
            assert a.shape[1] == whole_frames                # the push that crosses the mark releases all of them
            released = True
        outs.append(a)
    toks = torch.cat(outs, 1)
    assert toks.shape[1] == rs.emitted // hop and s.pending == rs.emitted % hop
    with pytest.raises(ValueError, match="finish"):
        s.push(sig[:, :5])
    return toks, rs.emitted


def test_encodec_encode_stream_resamples(encodecs):
    from oracle import encodec_oracle as O

    cfg, sd, c16, c24 = encodecs
    total, sizes = sizes_16k(E_HOP, (7, 0, 213, 1, 320, 2, 900))
    sig = noise(701, 2, total)
    toks, emitted = encode_both_ways(c16, c24, sig.cuda(), sizes, E_HOP, WARMUP)
    frames = toks.shape[1]
    assert emitted == math.ceil(3 * total / 2) and frames == FRAMES and emitted % E_HOP > 0
    one_shot = c16.sig_to_toks(sig.cuda())[:, :frames]
    sig24 = torch.from_numpy(R.resample(sig.numpy().astype(np.float64), 16000, 24000)[:, : frames * E_HOP])
    with torch.no_grad():
        _, m64 = O.sig_to_toks(cfg, O.fold_weight_norm(sd, torch.float64), sig24, None, 8, True)
    encodec_check_tokens("tiny_16k/resample", toks, one_shot.cpu().numpy(), m64.numpy())


def test_mimi_encode_stream_resamples(mimis):
    from oracle import mimi_oracle as O

    cfg, sd, c16, c24 = mimis
    total, sizes = sizes_16k(M_HOP, (7, 0, 213, 1, 1280, 2, 2900))
    sig = noise(702, 2, total)
    toks, emitted = encode_both_ways(c16, c24, sig.cuda(), sizes, M_HOP, 0)
    frames = toks.shape[1]
    assert emitted == math.ceil(3 * total / 2) and frames == FRAMES and emitted % M_HOP > 0
    one_shot = c16.sig_to_toks(sig.cuda())[:, :frames]
    sig24 = torch.from_numpy(R.resample(sig.numpy().astype(np.float64), 16000, 24000)[:, : frames * M_HOP])
    with torch.no_grad():
        _, m64 = O.sig_to_toks(cfg, O.cast_weights(sd, torch.float64), sig24, None, c16.num_codebooks, True)
    mimi_check_tokens(toks, one_shot.cpu().numpy(), m64.numpy())


def rand_toks(seed, N, K, vocab):
    from audiocodecs_amd import prng

    return torch.from_numpy(prng.randint(seed, "rstream", (2, N, K), vocab)).to(torch.int64).cuda()


@pytest.mark.parametrize("which", ["encodec", "mimi"])
def test_decode_stream_resamples(which, request):
    from audiocodecs_amd.resample import resample

    cfg, sd, c16, c24 = request.getfixturevalue("encodecs" if which == "encodec" else "mimis")
    toks = rand_toks(703, FRAMES, c16.num_codebooks, c16.vocab_size)
    sizes = cycled((1, 0, 3, 2, 7), FRAMES)
    s, plain = c16.decode_stream(2, resample=True), c24.decode_stream(2)
    outs, plains, t = [], [], 0
    for n in sizes:
        outs.append(s.push(toks[:, t:t + n]))
        plains.append(plain.push(toks[:, t:t + n]))
        t += n
    outs.append(s.finish())
    got, at24 = torch.cat(outs, 1), torch.cat(plains, 1)
    assert at24.shape[1] == FRAMES * c24.config.hop_length
    assert torch.equal(got, resample(at24, 24000, 16000))
    assert got.shape[1] == c16.toks_to_sig(toks).shape[1] == math.ceil(2 * at24.shape[1] / 3)
    with pytest.raises(ValueError, match="finish"):
        s.push(toks[:, :1])
    s.reset()                                                                   # both halves start over
    again = [s.push(toks[:, a:a + n]) for a, n in zip(np.cumsum([0] + sizes[:-1]), sizes)] + [s.finish()]
    assert torch.equal(torch.cat(again, 1), got)


@pytest.mark.parametrize("which", ["encodec", "mimi"])
def test_keyword_behaviour(which, request):
    cfg, sd, c16, c24 = request.getfixturevalue("encodecs" if which == "encodec" else "mimis")
    hop = c24.config.hop_length
    sig = noise(704, 2, 9 * hop + 11).cuda()
    toks = rand_toks(705, 9, c24.num_codebooks, c24.vocab_size)
    # equal rates: the plain stream
    a, b = c24.encode_stream(2, resample=True), c24.encode_stream(2)
    assert a._rs is None
    for lo, hi in ((0, 100), (100, 8 * hop), (8 * hop, sig.shape[1])):
        assert torch.equal(a.push(sig[:, lo:hi]), b.push(sig[:, lo:hi]))
    assert a.finish().shape == (2, 0, c24.num_codebooks) and a.pending == b.pending == 11
    d, e = c24.decode_stream(2, resample=True), c24.decode_stream(2)
    assert torch.equal(torch.cat([d.push(toks[:, :8]), d.push(toks[:, 8:])], 1), torch.cat([e.push(toks[:, :8]), e.push(toks[:, 8:])], 1))
    assert d.finish().shape == (2, 0)
    # the default keyword at another rate: refused as before
    for fn in (c16.encode_stream, c16.decode_stream):
        with pytest.raises(ValueError, match="resampling"):
            fn(2)
    # single slots cannot restart while resampling; the stream goes on
    s = c16.encode_stream(2, resample=True)
    first = s.push(sig[:, : 8 * hop])
    with pytest.raises(ValueError):
        s.reset(streams=[1])
    ref = c16.encode_stream(2, resample=True)
    assert torch.equal(ref.push(sig[:, : 8 * hop]), first)
    assert torch.equal(s.push(sig[:, 8 * hop:]), ref.push(sig[:, 8 * hop:])) and torch.equal(s.finish(), ref.finish())
    ds = c16.decode_stream(2, resample=True)
    with pytest.raises(ValueError):
        ds.reset(streams=[1])
    ds.reset()
    out = torch.cat([ds.push(toks), ds.finish()], 1)
    assert out.shape[1] == c16.toks_to_sig(toks).shape[1]
