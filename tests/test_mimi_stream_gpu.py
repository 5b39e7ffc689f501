"""Streaming Mimi encode on the GPU (Mimi.encode_stream, include/audiocodecs_amd.h ac_mimi_stream_*) against transformers'
streamed tokens (tests/golden/mimi_stream_golden.npz), the batch path, and itself.

Token bars as everywhere: equality wherever the fp64 margin of the frame clears TAU at this and earlier stages
(tests/test_oracle_golden.py); the bitwise checks compare the stream with itself and need no excuse."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from golden_cases import noise
from mimi_stream_cases import CASES, HOP, make_signal
from test_oracle_golden import tokens_match_up_to_ties

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_ENOMEM = -1, -3


@pytest.fixture(scope="module")
def stream_golden():
    z = np.load(os.path.join(GOLDEN_DIR, "mimi_stream_golden.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


@pytest.fixture(scope="module")
def codecs(mimi_checkpoints):
    from audiocodecs_amd import Mimi

    cache = {}

    def get(cfg_name, seed=0, precision=None, **kw):
        key = (cfg_name, seed, precision, tuple(sorted(kw.items())))
        if key not in cache:
            cfg, sd = mimi_checkpoints(cfg_name, seed)
            cache[key] = Mimi(24000, state_dict=sd, config=cfg, precision=precision, **kw).eval()
        return cache[key]

    return get


def run_schedule(stream, sig, sizes):
    """Push sig [B, T] (cuda) in pieces of `sizes` samples; returns the concatenated tokens and checks `pending` each time."""
    out, t = [], 0
    for n in sizes:
        before = stream.pending
        toks = stream.push(sig[:, t:t + n])
        t += n
        assert toks.dtype == torch.int64 and toks.shape == (sig.shape[0], (before + n) // HOP, stream.num_codebooks)
        assert stream.pending == (before + n) % HOP
        out.append(toks)
    return torch.cat(out, 1)


def check_tokens(toks, gold, margin):
    n, bad, excused = tokens_match_up_to_ties(toks.cpu().numpy(), gold.astype(np.int64), margin)
    assert bad == 0, f"{bad} of {n} tokens differ outside near-ties ({excused} excused)"
    assert n > 0.8 * gold.size, (n, excused)     # (full Mimi: ~10 % of the tokens sit behind a near-tie)


def case_of(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_case_in_its_schedule(case, stream_golden, codecs):
    z, meta = stream_golden
    info = meta["cases"][case["name"]]
    codec = codecs(case["cfg"], case["weights_seed"])
    sig = torch.from_numpy(make_signal(case, GOLDEN_DIR)).cuda()
    s = codec.encode_stream(info["B"])
    toks = run_schedule(s, sig, [n * HOP for n in info["pushes"]])
    assert s.pending == 0
    check_tokens(toks, z[f"{case['name']}_stream"], z[f"{case['name']}_margin"])


def test_long_tiny_stream_passes_the_rope_table(stream_golden, codecs):
    """8 320 transformer positions: the stream goes on where the batch path's 8 192-row RoPE table ends."""
    from audiocodecs_amd._native import NativeError

    z, meta = stream_golden
    case = case_of("tiny_long")
    assert 2 * meta["cases"]["tiny_long"]["frames"] > 8192
    codec = codecs("tiny")
    sig = torch.from_numpy(make_signal(case, GOLDEN_DIR)).cuda()
    with pytest.raises(NativeError, match="RoPE|too long"):     # (the per-call sample limit comes first)
        codec.sig_to_toks(sig)
    s = codec.encode_stream(1)
    toks = run_schedule(s, sig, [64 * HOP] * (sig.shape[1] // (64 * HOP)))
    check_tokens(toks, z["tiny_long_stream"], z["tiny_long_margin"])


@pytest.mark.parametrize("name", ["tiny_b3_f40", "full_ragged"])
def test_sub_frame_pushes(name, stream_golden, codecs):
    z, meta = stream_golden
    case = case_of(name)
    codec = codecs(case["cfg"], case["weights_seed"])
    sig = torch.from_numpy(make_signal(case, GOLDEN_DIR)).cuda()
    T = sig.shape[1]
    sizes = [1, 7, 0, 1913, 3845]
    rng = np.random.default_rng(7)
    while sum(sizes) < T:
        sizes.append(int(min(rng.integers(0, 3 * HOP), T - sum(sizes))))
    s = codec.encode_stream(sig.shape[0])
    toks = run_schedule(s, sig, sizes)
    assert s.pending == 0 and toks.shape[1] == T // HOP
    check_tokens(toks, z[f"{name}_stream"], z[f"{name}_margin"])


@pytest.mark.parametrize("precision", ["fp32", "fp32_exact"])
def test_stream_agrees_with_batch_path(precision, stream_golden, codecs):
    z, meta = stream_golden
    case = case_of("full_b2_f160")
    codec = codecs("full", 0, precision)
    n = 30
    sig = torch.from_numpy(make_signal(case, GOLDEN_DIR)[:, : n * HOP]).cuda()
    batch = codec.sig_to_toks(sig)
    s = codec.encode_stream(2)
    toks = run_schedule(s, sig, [3 * HOP] * (n // 3))
    check_tokens(toks, batch.cpu().numpy(), z["full_b2_f160_margin"][:, :n])
    check_tokens(toks, z["full_b2_f160_stream"][:, :n], z["full_b2_f160_margin"][:, :n])


def test_streams_are_isolated_bitwise(codecs):
    codec = codecs("full")
    n = 12
    x = noise(401, 1, n * HOP).cuda()
    other = noise(402, 1, n * HOP).cuda()
    alone = run_schedule(codec.encode_stream(1), x, [2 * HOP] * (n // 2))
    for fill in (other, torch.full_like(x, float("nan"))):
        batch = torch.cat([fill, x, other * 3.0], 0)
        got = run_schedule(codec.encode_stream(3), batch, [2 * HOP] * (n // 2))
        assert torch.equal(got[1:2], alone)


def test_reset_reruns_bitwise(codecs):
    codec = codecs("full")
    sig = noise(403, 2, 9 * HOP).cuda()
    s = codec.encode_stream(2)
    first = run_schedule(s, sig, [HOP, 3 * HOP + 5, 5 * HOP - 5])
    s.reset()
    assert s.pending == 0
    again = run_schedule(s, sig, [HOP, 3 * HOP + 5, 5 * HOP - 5])
    assert torch.equal(first, again)


def test_reset_one_slot_mid_stream(codecs):
    codec = codecs("full")
    a = noise(404, 3, 8 * HOP).cuda()
    b = noise(405, 3, 6 * HOP).cuda()
    plain = codec.encode_stream(3)
    p1 = run_schedule(plain, a, [2 * HOP] * 4)
    p2 = run_schedule(plain, b, [2 * HOP] * 3)
    s = codec.encode_stream(3)
    s1 = run_schedule(s, a, [2 * HOP] * 4)
    s.reset([1])
    s2 = run_schedule(s, b, [2 * HOP] * 3)
    assert torch.equal(s1, p1)
    assert torch.equal(s2[[0, 2]], p2[[0, 2]])          # the other slots never notice
    fresh = run_schedule(codec.encode_stream(3), b, [2 * HOP] * 3)
    assert torch.equal(s2[1], fresh[1])                  # slot 1 restarted from nothing


def test_python_errors(codecs, mimi_checkpoints):
    from audiocodecs_amd import Mimi

    cfg, sd = mimi_checkpoints("tiny", 0)
    with pytest.raises(ValueError, match="decode"):
        Mimi(24000, mode="decode", state_dict=sd, config=cfg).encode_stream(1)
    with pytest.raises(ValueError, match="resampling"):
        Mimi(16000, state_dict=sd, config=cfg).encode_stream(1)
    codec = codecs("tiny")
    for bad in (0, -2, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            codec.encode_stream(bad)
    s = codec.encode_stream(2)
    x = noise(406, 2, 3 * HOP).cuda()
    for bad in (x[:1], x[0], x.double(), x.cpu(), x[:, None]):
        with pytest.raises(ValueError):
            s.push(bad)
    s.push(x[:, :100])
    with pytest.raises(ValueError, match="pending"):
        s.reset([0])
    s.reset()
    with pytest.raises(ValueError):
        s.reset([2])
    # the stream still works after every refusal
    toks = s.push(x)
    ref = codec.encode_stream(2).push(x)
    assert torch.equal(toks, ref)


def test_abi_errors_leave_the_handle_usable(codecs, checkpoints):
    from audiocodecs_amd import Encodec
    from audiocodecs_amd.encodec import _ptr, _stream

    codec = codecs("tiny")
    B, F, K = 2, 2, codec.num_codebooks
    x = noise(407, B, F * HOP).cuda()
    keep = codec.encode_stream(B)          # (kept alive: the handle knows reset states by address, and a freed one's could come back)
    want = keep.push(x)
    nat = codec._native_for(x)
    L, h = nat.lib, nat.h
    nbytes = L.ac_mimi_stream_state_bytes(h, B)
    wsb = L.ac_mimi_stream_workspace_bytes(h, B, F)
    assert nbytes > 0 and wsb > 0
    state = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    toks = torch.empty(B, F, K, dtype=torch.int64, device=x.device)

    def enc(st=state, sb=nbytes, b=B, w=ws, wb=wsb):
        return L.ac_mimi_stream_encode(h, _ptr(st), sb, _ptr(x), b, F, K, _ptr(toks), _ptr(w), wb, _stream())

    assert enc() == AC_EINVAL                                               # never reset
    mask = torch.ones(B, dtype=torch.uint8, device=x.device)
    assert L.ac_mimi_stream_reset(h, _ptr(state), nbytes, B, _ptr(mask), _stream()) == AC_EINVAL   # first reset takes no mask
    assert L.ac_mimi_stream_reset(h, _ptr(state), nbytes - 256, B, None, _stream()) == AC_ENOMEM
    assert L.ac_mimi_stream_reset(h, _ptr(state), nbytes, B, None, _stream()) == 0
    assert enc(sb=nbytes - 256) == AC_ENOMEM                                # state too small
    assert enc(wb=wsb - 4096) == AC_ENOMEM                                  # workspace too small
    assert enc(b=1) == AC_EINVAL                                            # reset for another B
    other = codecs("tiny", 1)                                               # another handle: never reset there
    onat = other._native_for(x)
    assert onat.lib.ac_mimi_stream_encode(onat.h, _ptr(state), nbytes, _ptr(x), B, F, K, _ptr(toks), _ptr(ws), wsb, _stream()) == AC_EINVAL
    assert enc() == 0
    torch.cuda.synchronize()
    assert torch.equal(toks, want)                                          # the refusals changed nothing
    # a non-Mimi handle
    ecfg, esd = checkpoints("tiny", 0)
    e = Encodec(24000, num_codebooks=2, state_dict=esd, config=ecfg)
    enat = e._native_for(x)
    assert L.ac_mimi_stream_state_bytes(enat.h, B) == 0
    assert L.ac_mimi_stream_reset(enat.h, _ptr(state), nbytes, B, None, _stream()) == AC_EINVAL
    assert codec.encode_stream(B).push(x).equal(want)
