"""Streaming Mimi decode on the GPU (Mimi.decode_stream, include/audiocodecs_amd.h ac_mimi_stream_decode*).

The decoder is causal, so the one-shot decode of a token sequence is the oracle of every push schedule
(tests/test_mimi_dstream.py): the stream is compared with the reference's one-shot waveform (tests/golden/mimi_golden.npz), with
the fp64 oracle next to the batch path (`toks_to_sig`), and bitwise with itself.  The linear layers of a push have two routes
(ac_debug_set "mstream_skinny": 0 = tap-GEMM, 1 = mstream_linear_kernel); the bitwise tests force one so both sides take the same."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from mimi_cases import REC_STRIDE
from mimi_dstream_cases import NAMES, SCHEDULES, case_of, schedule, tokens_of
from test_gpu_parity import rms
import parity_record

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_ENOMEM = -1, -3
BAR = 1e-4          # waveform RMS error against the reference: the project's north-star bar (tests/test_mimi_gpu_parity.py)


@pytest.fixture(scope="module")
def codecs(mimi_checkpoints):
    from audiocodecs_amd import Mimi

    cache = {}

    def get(cfg_name, seed=0, K=8, **kw):
        key = (cfg_name, seed, K, tuple(sorted(kw.items())))
        if key not in cache:
            cfg, sd = mimi_checkpoints(cfg_name, seed)
            cache[key] = Mimi(24000, num_codebooks=K, state_dict=sd, config=cfg, **kw).eval()
        return cache[key]

    return get


def set_route(codec, value):
    from audiocodecs_amd import _native

    codec._native_for(torch.empty(0, device="cuda"))
    _native.debug_set(codec, "mstream_skinny", value)


def run_schedule(stream, toks, sizes):
    """Push toks [B, N, K] (cuda) in pieces of `sizes` frames; returns the concatenated samples."""
    out, t = [], 0
    for n in sizes:
        sig = stream.push(toks[:, t:t + n])
        assert sig.dtype == torch.float32 and sig.shape == (toks.shape[0], n * stream.hop)
        t += n
        out.append(sig)
    assert t == toks.shape[1]
    return torch.cat(out, 1)


def codec_for(name, mimi_golden, codecs):
    z, meta = mimi_golden
    case = case_of(name)
    return codecs(case["cfg"], case["weights_seed"], meta["cases"][name]["K"])


# ---- 3. the reference's one-shot waveform -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SCHEDULES))
@pytest.mark.parametrize("name", NAMES)
def test_stream_matches_the_reference_one_shot_decode(name, kind, mimi_golden, codecs):
    z, meta = mimi_golden
    codec = codec_for(name, mimi_golden, codecs)
    set_route(codec, -1)
    toks = tokens_of(name, z, GOLDEN_DIR).cuda()
    if name == "full_example":
        assert codec.config.resample_stride * toks.shape[1] > codec.config.sliding_window      # the ring wraps
    s = codec.decode_stream(toks.shape[0])
    rec = run_schedule(s, toks, schedule(kind, toks.shape[1])).cpu().numpy()
    assert list(rec.shape) == meta["cases"][name]["rec_shape"]
    err = rms(rec.reshape(-1)[::REC_STRIDE] - z[f"{name}.rec_strided"])
    parity_record.record("mimi_dstream", f"{name}/{kind}", waveform_rms_err=err)
    print(f"mimi_dstream {name}/{kind}: waveform RMS error {err:.3e}")
    assert err < BAR, err


# ---- 4. against the batch path, both against the fp64 oracle -------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle64(mimi_golden, mimi_checkpoints):
    """name -> the fp64 oracle's one-shot decode of the case's tokens (numpy float64)."""
    from oracle import mimi_oracle as O

    z, meta = mimi_golden
    out, weights = {}, {}
    for name in NAMES:
        case = case_of(name)
        key = (case["cfg"], case["weights_seed"])
        if key not in weights:
            cfg, sd = mimi_checkpoints(*key)
            weights[key] = (cfg, O.cast_weights(sd, torch.float64))
        cfg, W64 = weights[key]
        with torch.no_grad():
            out[name] = O.toks_to_sig(cfg, W64, tokens_of(name, z, GOLDEN_DIR)).numpy()
    return out


@pytest.mark.parametrize("route", [0, 1])
def test_stream_error_is_of_the_batch_paths_size(route, mimi_golden, codecs, oracle64):
    """Pooled over every sample of every case (one RMS each, so a short case cannot tip it): the stream's error against the fp64
    oracle must not exceed twice the batch path's.  Both evaluate the same graph in the same arithmetic with different tile shapes
    and scale granularity: their rounding noise is of one size and independent, and a factor of two covers that and nothing else."""
    z, meta = mimi_golden
    se, be = [], []
    for name in NAMES:
        codec = codec_for(name, mimi_golden, codecs)
        toks = tokens_of(name, z, GOLDEN_DIR).cuda()
        ref = oracle64[name]
        be.append((codec.toks_to_sig(toks).cpu().numpy().astype(np.float64) - ref).reshape(-1))
        set_route(codec, route)
        for kind in SCHEDULES:
            rec = run_schedule(codec.decode_stream(toks.shape[0]), toks, schedule(kind, toks.shape[1]))
            se.append((rec.cpu().numpy().astype(np.float64) - ref).reshape(-1))
        set_route(codec, -1)
    s_rms, b_rms = rms(np.concatenate(se)), rms(np.concatenate(be))
    parity_record.record("mimi_dstream", f"pooled_vs_fp64/route{route}", stream_rms_err=s_rms, batch_rms_err=b_rms)
    print(f"mimi_dstream route {route}: pooled RMS error against fp64: stream {s_rms:.3e}, batch path {b_rms:.3e}")
    assert b_rms > 0
    assert s_rms <= 2.0 * b_rms, (s_rms, b_rms)


# ---- 5. a stream longer than the batch path takes --------------------------------------------------------------------------------
def test_long_stream_decodes_past_the_batch_paths_limit(codecs, mimi_checkpoints):
    """4 160 frames = 8 320 transformer positions, 64 frames per push, against the fp32 oracle's one-shot decode on the CPU."""
    from audiocodecs_amd._native import NativeError
    from oracle import mimi_oracle as O

    z = np.load(os.path.join(GOLDEN_DIR, "mimi_stream_golden.npz"))
    toks = torch.from_numpy(z["tiny_long_stream"].astype(np.int64))
    assert toks.shape[0] == 1 and 2 * toks.shape[1] > 8192
    cfg, sd = mimi_checkpoints("tiny", 0)
    codec = codecs("tiny", 0, toks.shape[2])
    set_route(codec, -1)
    with pytest.raises(NativeError, match="RoPE|too long"):
        codec.toks_to_sig(toks.cuda())
    s = codec.decode_stream(1)
    rec = run_schedule(s, toks.cuda(), [64] * (toks.shape[1] // 64)).cpu().numpy()
    with torch.no_grad():
        ref = O.toks_to_sig(cfg, O.cast_weights(sd), toks).numpy()
    assert rec.shape == ref.shape
    err, tail = rms(rec - ref), rms(rec[:, -256 * 1920:] - ref[:, -256 * 1920:])
    parity_record.record("mimi_dstream", "tiny_long_stream", waveform_rms_err=err)
    print(f"mimi_dstream tiny_long_stream: RMS error {err:.3e} (last 256 frames {tail:.3e}), signal RMS {rms(ref):.3e}")
    assert err < BAR and tail < BAR, (err, tail)


# ---- 6. one-frame pushes from a fresh state ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
def test_one_frame_pushes_from_fresh_equal_one_push(route, mimi_golden, codecs):
    """F = 1 from a fresh state brings 2 rows to the first conv, whose history holds 6: every push of the first three goes through the
    short-chunk staging with a history that is part zeros, part cache.  Eight of them against one F = 8 push."""
    z, meta = mimi_golden
    codec = codecs("full")
    set_route(codec, route)
    toks = tokens_of("full_noise_b2", z, GOLDEN_DIR)[:, :8].cuda()
    assert toks.shape[1] == 8
    one = run_schedule(codec.decode_stream(2), toks, [8]).cpu().numpy()
    eight = run_schedule(codec.decode_stream(2), toks, [1] * 8).cpu().numpy()
    set_route(codec, -1)
    gold = z["full_noise_b2.rec_strided"]
    n = one.size
    idx = np.arange(0, meta["cases"]["full_noise_b2"]["rec_shape"][1] * 2, REC_STRIDE)      # strided positions of the [2, N*hop] fixture ...
    b, t = idx // meta["cases"]["full_noise_b2"]["rec_shape"][1], idx % meta["cases"]["full_noise_b2"]["rec_shape"][1]
    keep = t < one.shape[1]                                                                  # ... that fall inside the first 8 frames
    for got, what in ((one, "F=8"), (eight, "8 x F=1")):
        err = rms(got[b[keep], t[keep]] - gold[keep])
        print(f"mimi_dstream route {route} {what}: RMS error against the reference {err:.3e}")
        assert err < BAR, (what, err)
    d = rms(one - eight)
    print(f"mimi_dstream route {route}: RMS of (F=8 push) - (8 x F=1 pushes) {d:.3e}")
    assert d < BAR, d
    assert n == 2 * 8 * 1920


# ---- 7. bitwise properties of the stream with itself -------------------------------------------------------------------------------
def rand_toks(seed, B, N, K=8):
    from audiocodecs_amd import prng

    return torch.from_numpy(prng.randint(seed, "dstream", (B, N, K), 2048)).to(torch.int64).cuda()


@pytest.mark.parametrize("route", [0, 1])
def test_streams_are_isolated_bitwise(route, codecs):
    codec = codecs("full")
    set_route(codec, route)
    x, a, b = rand_toks(501, 1, 12), rand_toks(502, 1, 12), rand_toks(503, 1, 12)
    for sizes in ([2] * 6, [1] * 12):
        alone = run_schedule(codec.decode_stream(1), x, sizes)
        got = run_schedule(codec.decode_stream(3), torch.cat([a, x, b], 0), sizes)
        assert torch.equal(got[1:2], alone)
    set_route(codec, -1)


@pytest.mark.parametrize("route", [0, 1])
def test_reset_reruns_bitwise(route, codecs):
    codec = codecs("full")
    set_route(codec, route)
    toks = rand_toks(504, 2, 9)
    s = codec.decode_stream(2)
    first = run_schedule(s, toks, [1, 3, 5])
    s.reset()
    again = run_schedule(s, toks, [1, 3, 5])
    set_route(codec, -1)
    assert torch.equal(first, again)


@pytest.mark.parametrize("route", [0, 1])
def test_reset_one_slot_mid_stream(route, codecs):
    codec = codecs("full")
    set_route(codec, route)
    a, b = rand_toks(505, 3, 8), rand_toks(506, 3, 6)
    plain = codec.decode_stream(3)
    p1 = run_schedule(plain, a, [2] * 4)
    p2 = run_schedule(plain, b, [2] * 3)
    s = codec.decode_stream(3)
    s1 = run_schedule(s, a, [2] * 4)
    s.reset([1])
    s2 = run_schedule(s, b, [2] * 3)
    fresh = run_schedule(codec.decode_stream(3), b, [2] * 3)
    set_route(codec, -1)
    assert torch.equal(s1, p1)
    assert torch.equal(s2[[0, 2]], p2[[0, 2]])          # the other slots never notice
    assert torch.equal(s2[1], fresh[1])                  # slot 1 restarted from nothing
    assert not torch.equal(s2[1], p2[1])


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [0, 1])
def test_a_captured_push_replays_on_new_tokens(route, codecs):
    """Position and `fresh` live on the device: one captured F-frame push, replayed on new tokens for consecutive frames, is the eager
    stream bit for bit."""
    codec = codecs("full")
    set_route(codec, route)
    B, F, n = 2, 1, 7
    toks = rand_toks(507, B, F * n)
    eager = run_schedule(codec.decode_stream(B), toks, [F] * n)
    s = codec.decode_stream(B)
    s.push(toks[:, :F])                                  # the workspace exists before the capture
    s.reset()
    torch.cuda.synchronize()
    tx = toks[:, :F].clone()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            sig = s.push(tx)
    s.reset()                                            # (capturing ran nothing; start from position 0 all the same)
    out = []
    for i in range(n):
        tx.copy_(toks[:, i * F:(i + 1) * F])
        g.replay()
        torch.cuda.synchronize()
        out.append(sig.clone())
    set_route(codec, -1)
    assert torch.equal(torch.cat(out, 1), eager)


# ---- 9. errors -----------------------------------------------------------------------------------------------------------------------
def test_python_errors(codecs, mimi_checkpoints):
    from audiocodecs_amd import Mimi, MimiDecodeStream

    cfg, sd = mimi_checkpoints("tiny", 0)
    with pytest.raises(ValueError, match="encode"):
        Mimi(24000, mode="encode", state_dict=sd, config=cfg).decode_stream(1)
    with pytest.raises(ValueError, match="resampling"):
        Mimi(16000, state_dict=sd, config=cfg).decode_stream(1)
    codec = codecs("tiny")
    for bad in (0, -2, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            codec.decode_stream(bad)
    s = codec.decode_stream(2)
    assert isinstance(s, MimiDecodeStream) and s.MAX_POSITIONS == 1 << 24
    x = rand_toks(508, 2, 3)
    for bad in (x[:1], x[0], x.int(), x.float(), x.cpu(), x[:, :, :4], x[:, None]):
        with pytest.raises(ValueError):
            s.push(bad)
    with pytest.raises(ValueError):
        s.reset([2])
    empty = s.push(x[:, :0])
    assert empty.shape == (2, 0) and empty.dtype == torch.float32
    sig = s.push(x)                                      # the stream still works after every refusal
    assert torch.equal(sig, codec.decode_stream(2).push(x))


def test_abi_errors_leave_the_handle_usable(codecs, checkpoints):
    from audiocodecs_amd import Encodec
    from audiocodecs_amd.encodec import _ptr, _stream

    codec = codecs("tiny")
    B, F, K = 2, 2, codec.num_codebooks
    x = rand_toks(509, B, F)
    keep = codec.decode_stream(B)          # (kept alive: the handle knows reset states by address, and a freed one's could come back)
    want = keep.push(x)
    nat = codec._native_for(x)
    L, h = nat.lib, nat.h
    hop = codec.config.hop_length
    nbytes = L.ac_mimi_stream_decode_state_bytes(h, B)
    wsb = L.ac_mimi_stream_decode_workspace_bytes(h, B, F)
    ebytes = L.ac_mimi_stream_state_bytes(h, B)
    ewsb = L.ac_mimi_stream_workspace_bytes(h, B, F)
    assert nbytes > 0 and wsb > 0 and ebytes > 0
    big = max(nbytes, ebytes)
    state = torch.empty(big, dtype=torch.uint8, device=x.device)
    estate = torch.empty(big, dtype=torch.uint8, device=x.device)
    ws = torch.empty(max(wsb, ewsb), dtype=torch.uint8, device=x.device)
    sig = torch.empty(B, F * hop, dtype=torch.float32, device=x.device)
    esig = torch.zeros(B, F * hop, dtype=torch.float32, device=x.device)
    etoks = torch.empty(B, F, K, dtype=torch.int64, device=x.device)

    def dec(st=state, sb=nbytes, b=B, w=ws, wb=wsb):
        return L.ac_mimi_stream_decode(h, _ptr(st), sb, _ptr(x), b, F, K, _ptr(sig), _ptr(w), wb, _stream())

    assert dec() == AC_EINVAL                                               # never reset
    mask = torch.ones(B, dtype=torch.uint8, device=x.device)
    assert L.ac_mimi_stream_decode_reset(h, _ptr(state), nbytes, B, _ptr(mask), _stream()) == AC_EINVAL   # first reset takes no mask
    assert L.ac_mimi_stream_decode_reset(h, _ptr(state), nbytes - 256, B, None, _stream()) == AC_ENOMEM
    assert L.ac_mimi_stream_decode_reset(h, _ptr(state), nbytes, B, None, _stream()) == 0
    assert dec(sb=nbytes - 256) == AC_ENOMEM                                # state too small
    assert dec(wb=wsb - 4096) == AC_ENOMEM                                  # workspace too small
    assert dec(b=1) == AC_EINVAL                                            # reset for another B
    other = codecs("tiny", 1)                                               # another handle: never reset there
    onat = other._native_for(x)
    assert onat.lib.ac_mimi_stream_decode(onat.h, _ptr(state), nbytes, _ptr(x), B, F, K, _ptr(sig), _ptr(ws), wsb, _stream()) == AC_EINVAL
    # an encode state where a decode state is expected, and the reverse
    assert L.ac_mimi_stream_reset(h, _ptr(estate), ebytes, B, None, _stream()) == 0
    assert dec(st=estate, sb=big) == AC_EINVAL
    assert L.ac_mimi_stream_decode_reset(h, _ptr(estate), big, B, _ptr(mask), _stream()) == AC_EINVAL
    assert L.ac_mimi_stream_encode(h, _ptr(state), big, _ptr(esig), B, F, K, _ptr(etoks), _ptr(ws), ws.numel(), _stream()) == AC_EINVAL
    assert L.ac_mimi_stream_reset(h, _ptr(state), big, B, _ptr(mask), _stream()) == AC_EINVAL
    assert L.ac_mimi_stream_encode(h, _ptr(estate), ebytes, _ptr(esig), B, F, K, _ptr(etoks), _ptr(ws), ws.numel(), _stream()) == 0     # each still is what it was
    assert dec() == 0
    torch.cuda.synchronize()
    assert torch.equal(sig, want)                                           # the refusals changed nothing
    # a non-Mimi handle
    ecfg, esd = checkpoints("tiny", 0)
    e = Encodec(24000, num_codebooks=2, state_dict=esd, config=ecfg)
    xnat = e._native_for(x)
    assert L.ac_mimi_stream_decode_state_bytes(xnat.h, B) == 0
    assert L.ac_mimi_stream_decode_workspace_bytes(xnat.h, B, F) == 0
    assert L.ac_mimi_stream_decode_reset(xnat.h, _ptr(state), nbytes, B, None, _stream()) == AC_EINVAL
    assert codec.decode_stream(B).push(x).equal(want)


def test_out_of_range_token_behaves_as_in_the_batch_decode(codecs):
    """NaN frame, sticky word, AC_EINVAL at the next call -- and the handle goes on working."""
    from audiocodecs_amd._native import NativeError

    codec = codecs("tiny")
    x = rand_toks(510, 1, 2)
    bad = x.clone()
    bad[0, 1, 0] = 4096
    s = codec.decode_stream(1)
    sig = s.push(bad)
    torch.cuda.synchronize()
    assert torch.isnan(sig[0, 1920:]).any() and not torch.isnan(sig[0, :1920]).any()
    with pytest.raises(NativeError, match="token"):
        s.push(x)
    s.reset()
    assert torch.equal(s.push(x), codec.decode_stream(1).push(x))
