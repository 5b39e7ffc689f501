"""Streaming EnCodec on the GPU (Encodec.encode_stream / decode_stream, include/audiocodecs_amd.h ac_encodec_stream_*).

EnCodec is causal, so once a stream has held back its first 7 frames the reference's one-shot result is the oracle of every push
schedule (tests/test_encodec_stream_oracle.py): the streams are compared with the reference's fixtures
(tests/golden/encodec_golden.npz), with the fp64 oracle next to the batch path, and bitwise with themselves.  A stream is NOT
bit-equal to the batch path -- its split16 scales are taken per stream over a push, not over the clip -- which is why the
comparisons are against the oracle.

Token bars as everywhere: equality wherever the fp64 margin of the frame clears TAU at this and earlier stages
(tests/test_oracle_golden.py).  Waveform bar: what tests/test_gpu_parity.py::test_golden_fixture asserts of the batch path on the same
fixtures, read from that test (WAVE_BAR below) instead of restated here."""
import inspect
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from encodec_stream_cases import DECODE_ONLY, ENCODE_FRAMES, HOP, SCHEDULES, WARMUP, case_of, schedule, signal_of, tokens_of
from golden_cases import REC_STRIDE, noise, read_example_wav
from test_gpu_parity import capture, rms, test_golden_fixture as _batch_fixture_test
from test_oracle_golden import TAU, tokens_match_up_to_ties
import parity_record

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_ENOMEM = -1, -3
# every `assert rms(err) < BAR` the batch path's fixture test applies to its decoded waveform; the stream must clear all of them
_BARS = [float(m) for m in re.findall(r"assert rms\(err\) < ([0-9.e+-]+), rms\(err\)", inspect.getsource(_batch_fixture_test))]
assert _BARS, "tests/test_gpu_parity.py::test_golden_fixture no longer states its waveform bar where this file reads it"
WAVE_BAR = min(_BARS)


@pytest.fixture(scope="module")
def codecs(checkpoints):
    from audiocodecs_amd import Encodec

    cache = {}

    def get(cfg_name, seed=0, K=8, precision=None):
        key = (cfg_name, seed, K, precision)
        if key not in cache:
            cfg, sd = checkpoints(cfg_name, seed)
            cache[key] = Encodec(24000, num_codebooks=K, state_dict=sd, config=cfg, precision=precision).eval()
        return cache[key]

    return get


def codec_for(name, golden, codecs, precision=None):
    z, meta = golden
    case = case_of(name)
    return codecs(case["cfg"], case["weights_seed"], meta["cases"][name]["K"], precision)


def run_encode(stream, sig, sizes):
    """Push sig [B, T] (cuda) in pieces of `sizes` samples; checks the shape and `pending` contract of every push (nothing comes out
    before WARMUP whole frames are in; then every completed frame does) and returns the concatenated tokens."""
    out, t = [], 0
    assert stream.WARMUP_FRAMES == WARMUP and stream.hop == HOP
    for n in sizes:
        before, ran = stream.pending, stream.frames
        toks = stream.push(sig[:, t:t + n])
        t += n
        whole = (before + n) // HOP
        want = 0 if (ran == 0 and whole < WARMUP) else whole
        assert toks.dtype == torch.int64 and toks.shape == (sig.shape[0], want, stream.num_codebooks), (toks.shape, want)
        assert stream.pending == before + n - want * HOP and stream.frames == ran + want
        out.append(toks)
    return torch.cat(out, 1)


def run_decode(stream, toks, sizes):
    """Push toks [B, N, K] (cuda) in pieces of `sizes` frames; same contract on `pending_frames`; returns the concatenated samples."""
    out, t = [], 0
    assert stream.WARMUP_FRAMES == WARMUP
    for n in sizes:
        before, ran = stream.pending_frames, stream.frames
        sig = stream.push(toks[:, t:t + n])
        t += n
        want = 0 if (ran == 0 and before + n < WARMUP) else before + n
        assert sig.dtype == torch.float32 and sig.shape == (toks.shape[0], want * HOP), (sig.shape, want)
        assert stream.pending_frames == before + n - want and stream.frames == ran + want
        out.append(sig)
    assert t == toks.shape[1]
    return torch.cat(out, 1)


def check_tokens(tag, toks, gold, margin):
    toks, gold = toks.cpu().numpy(), gold.astype(np.int64)
    assert toks.shape == gold.shape, (toks.shape, gold.shape)
    n, bad, excused = tokens_match_up_to_ties(toks, gold, margin, TAU)
    parity_record.tokens("encodec_stream", tag, toks, gold, margin, TAU)
    print(f"encodec_stream {tag}: {int((toks != gold).sum())} of {gold.size} tokens differ, {bad} outside near-ties, {excused} excused")
    assert bad == 0, f"{bad} of {n} tokens differ outside near-ties ({excused} excused)"
    assert n > 0.95 * gold.size, (n, excused)          # excused shares of these fixtures: 1.6 % and less


# ---- 1. encode against the reference's tokens --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("full_example", "one_frame"), ("full_example", "ragged")]
                         + [(n, k) for n in ("full_noise_b2", "full_tones_b2", "full_w1_noise") for k in SCHEDULES])
def test_encode_stream_matches_the_reference_tokens(name, kind, golden, codecs):
    z, meta = golden
    codec = codec_for(name, golden, codecs)
    F = ENCODE_FRAMES[name]
    sig = signal_of(name, GOLDEN_DIR).cuda()
    s = codec.encode_stream(sig.shape[0])
    toks = run_encode(s, sig, [n * HOP for n in schedule(kind, F)])
    assert s.pending == 0
    check_tokens(f"{name}/{kind}", toks, z[f"{name}.toks"][:, :F], z[f"{name}.margin64"][:, :F])


@pytest.mark.parametrize("name", ["full_noise_b2", "full_tones_b2"])
def test_sub_frame_pushes(name, golden, codecs):
    z, meta = golden
    codec = codec_for(name, golden, codecs)
    F = ENCODE_FRAMES[name]
    sig = signal_of(name, GOLDEN_DIR).cuda()
    T = sig.shape[1]
    sizes = [1, 7, 0, 313, 2241]
    rng = np.random.default_rng(7)
    while sum(sizes) < T:
        sizes.append(int(min(rng.integers(0, 3 * HOP), T - sum(sizes))))
    s = codec.encode_stream(sig.shape[0])
    toks = run_encode(s, sig, sizes)
    assert s.pending == 0 and toks.shape[1] == F
    check_tokens(f"{name}/sub_frame", toks, z[f"{name}.toks"][:, :F], z[f"{name}.margin64"][:, :F])


# ---- 2. decode against the reference's one-shot waveform ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [(n, k) for n in list(ENCODE_FRAMES) + DECODE_ONLY for k in SCHEDULES
                                       if (n, k) != ("full_example", "all_at_once")])      # (one 793-frame push is the batch shape)
def test_decode_stream_matches_the_reference_one_shot_decode(name, kind, golden, codecs):
    z, meta = golden
    codec = codec_for(name, golden, codecs)
    toks = tokens_of(name, z, GOLDEN_DIR).cuda()
    N = toks.shape[1]
    s = codec.decode_stream(toks.shape[0])
    rec = run_decode(s, toks, schedule(kind, N)).cpu().numpy()
    assert list(rec.shape) == meta["cases"][name]["rec_shape"] and s.pending_frames == 0
    err = rms(rec.reshape(-1)[::REC_STRIDE] - z[f"{name}.rec_strided"])
    parity_record.record("encodec_dstream", f"{name}/{kind}", waveform_rms_err=err)
    print(f"encodec_dstream {name}/{kind}: waveform RMS error {err:.3e} (bar {WAVE_BAR:g})")
    assert err < WAVE_BAR, err


# ---- 3. the stream's error is of the batch path's size -----------------------------------------------------------------------------
def stream_feats(codec, sig, sizes):
    """The features of every push of one schedule (test hook: the push's [B][n][H] block), as [B, N, H]."""
    s = codec.encode_stream(sig.shape[0])
    H = codec.config.hidden_size

    def go():
        return [int(t.shape[1]) for t in (s.push(sig[:, a:a + n]) for a, n in zip(np.cumsum([0] + sizes[:-1]), sizes))]

    ns, flat = capture(codec, go)
    out, off = [], 0
    for n in ns:
        if n:
            out.append(flat[off:off + sig.shape[0] * n * H].reshape(sig.shape[0], n, H))
            off += sig.shape[0] * n * H
    assert off == flat.size
    return np.concatenate(out, 1)


def test_stream_error_is_of_the_batch_paths_size(golden, codecs, checkpoints):
    """Pooled over every element of every case (one RMS each, so a short case cannot tip it): the stream's error against the fp64
    oracle must not exceed twice the batch path's, for the encoder's features and for the decoder's waveform.  Both paths evaluate
    the same graph in the same arithmetic with different tile shapes and scale granularity (per push instead of per clip): their
    rounding noise is of one size and independent, and a factor of two covers that and nothing else."""
    from oracle import encodec_oracle as O

    z, meta = golden
    W64 = {}
    fe_s, fe_b, wv_s, wv_b = [], [], [], []
    for name in list(ENCODE_FRAMES) + DECODE_ONLY:
        case = case_of(name)
        codec = codec_for(name, golden, codecs)
        key = (case["cfg"], case["weights_seed"])
        if key not in W64:
            W64[key] = O.fold_weight_norm(checkpoints(*key)[1], torch.float64)
        cfg = checkpoints(*key)[0]
        kinds = ["ragged"] if name == "full_example" else list(SCHEDULES)
        if name in ENCODE_FRAMES:
            sig = signal_of(name, GOLDEN_DIR)
            with torch.no_grad():
                ref = O.sig_to_feats(cfg, W64[key], sig.double()).numpy()
            fe_b.append((codec.sig_to_feats(sig.cuda()).cpu().numpy().astype(np.float64) - ref).reshape(-1))
            for kind in kinds:
                got = stream_feats(codec, sig.cuda(), [n * HOP for n in schedule(kind, ENCODE_FRAMES[name])])
                fe_s.append((got.astype(np.float64) - ref).reshape(-1))
        toks = tokens_of(name, z, GOLDEN_DIR)
        with torch.no_grad():
            ref = O.toks_to_sig(cfg, W64[key], toks).numpy()
        wv_b.append((codec.toks_to_sig(toks.cuda()).cpu().numpy().astype(np.float64) - ref).reshape(-1))
        for kind in kinds:
            rec = run_decode(codec.decode_stream(toks.shape[0]), toks.cuda(), schedule(kind, toks.shape[1]))
            wv_s.append((rec.cpu().numpy().astype(np.float64) - ref).reshape(-1))
    for what, se, be in (("feats", fe_s, fe_b), ("waveform", wv_s, wv_b)):
        s_rms, b_rms = rms(np.concatenate(se)), rms(np.concatenate(be))
        parity_record.record("encodec_stream", f"pooled_vs_fp64/{what}", stream_rms_err=s_rms, batch_rms_err=b_rms)
        print(f"encodec_stream {what}: pooled RMS error against fp64: stream {s_rms:.3e}, batch path {b_rms:.3e}")
        assert b_rms > 0
        assert s_rms <= 2.0 * b_rms, (what, s_rms, b_rms)


# ---- 4. a long stream: the carried h and c do not drift -----------------------------------------------------------------------------
def test_long_stream_does_not_drift(codecs, checkpoints):
    """2 400 frames (32 s) of the example clip tiled, one frame per push after the warm-up: the last 100 frames' tokens against the
    fp32 oracle's one-shot tokens (fp64 margins), and the stream decode of the oracle's tokens against its one-shot waveform."""
    from oracle import encodec_oracle as O

    cfg, sd = checkpoints("full", 0)
    codec = codecs("full", 0)
    N, tail = 2400, 100
    wav = read_example_wav(GOLDEN_DIR)
    sig = wav.repeat(1, -(-N * HOP // wav.shape[1]))[:, : N * HOP].contiguous()
    W, W64 = O.fold_weight_norm(sd), O.fold_weight_norm(sd, torch.float64)
    with torch.no_grad():
        otoks = O.sig_to_toks(cfg, W, sig)
        _, m64 = O.sig_to_toks(cfg, W64, sig.double(), None, 8, True)
        orec = O.toks_to_sig(cfg, W, otoks).numpy()
    toks = run_encode(codec.encode_stream(1), sig.cuda(), [HOP] * N)
    assert toks.shape == (1, N, 8)
    check_tokens("long_tail", toks[:, -tail:], otoks.numpy()[:, -tail:], m64.numpy()[:, -tail:])
    rec = run_decode(codec.decode_stream(1), otoks.cuda(), [1] * N).cpu().numpy()
    err = rms(rec[:, -tail * HOP:] - orec[:, -tail * HOP:])
    parity_record.record("encodec_dstream", "long_tail", waveform_rms_err=err)
    print(f"encodec_dstream long stream: waveform RMS error over the last {tail} frames {err:.3e} (bar {WAVE_BAR:g})")
    assert err < WAVE_BAR, err


# ---- 5. bitwise properties of the streams with themselves ---------------------------------------------------------------------------
def rand_toks(seed, B, N, K=8):
    from audiocodecs_amd import prng

    return torch.from_numpy(prng.randint(seed, "estream", (B, N, K), 1024)).to(torch.int64).cuda()


def test_streams_are_isolated_bitwise(codecs):
    codec = codecs("full")
    n = 12
    x, other = noise(601, 1, n * HOP).cuda(), noise(602, 1, n * HOP).cuda()
    tx, ta, tb = rand_toks(603, 1, n), rand_toks(604, 1, n), rand_toks(605, 1, n)
    for frames in ([7, 2, 2, 1], [12], [1] * 12):
        sizes = [f * HOP for f in frames]
        alone = run_encode(codec.encode_stream(1), x, sizes)
        for fill in (other, torch.full_like(x, float("nan"))):
            got = run_encode(codec.encode_stream(3), torch.cat([fill, x, other * 3.0], 0), sizes)
            assert torch.equal(got[1:2], alone)
        alone = run_decode(codec.decode_stream(1), tx, frames)
        got = run_decode(codec.decode_stream(3), torch.cat([ta, tx, tb], 0), frames)
        assert torch.equal(got[1:2], alone)


def test_reset_reruns_bitwise_and_drops_the_held_frames(codecs):
    codec = codecs("full")
    sig, toks = noise(606, 2, 11 * HOP).cuda(), rand_toks(607, 2, 11)
    sizes = [3 * HOP, 4 * HOP + 5, HOP - 5, 3 * HOP]
    s = codec.encode_stream(2)
    first = run_encode(s, sig, sizes)
    s.reset()
    assert s.pending == 0 and s.frames == 0
    again = run_encode(s, sig, sizes)
    assert first.shape[1] == 11 and torch.equal(first, again)
    # a reset during the warm-up drops what was held: the stream starts over with the next push
    s.reset()
    assert s.push(noise(608, 2, 5 * HOP + 9).cuda()).shape[1] == 0 and s.pending == 5 * HOP + 9
    s.reset()
    assert s.pending == 0
    assert torch.equal(run_encode(s, sig, sizes), first)
    with pytest.raises(ValueError, match="together"):
        s.reset(streams=[0])
    d = codec.decode_stream(2)
    dfirst = run_decode(d, toks, [2, 5, 1, 3])
    d.reset()
    assert torch.equal(run_decode(d, toks, [2, 5, 1, 3]), dfirst)
    d.reset()
    assert d.push(rand_toks(609, 2, 4)).shape[1] == 0 and d.pending_frames == 4
    d.reset()
    assert d.pending_frames == 0 and torch.equal(run_decode(d, toks, [2, 5, 1, 3]), dfirst)
    with pytest.raises(ValueError, match="together"):
        d.reset(streams=[0])


# ---- 6. exact fp32 products ---------------------------------------------------------------------------------------------------------
def test_fp32_exact_streams(golden, codecs):
    z, meta = golden
    name = "full_noise_b2"
    codec = codec_for(name, golden, codecs, "fp32_exact")
    F = ENCODE_FRAMES[name]
    sig = signal_of(name, GOLDEN_DIR).cuda()
    toks = run_encode(codec.encode_stream(2), sig, [n * HOP for n in schedule("ragged", F)])
    check_tokens(f"{name}/ragged/fp32_exact", toks, z[f"{name}.toks"][:, :F], z[f"{name}.margin64"][:, :F])
    gt = tokens_of(name, z, GOLDEN_DIR).cuda()
    rec = run_decode(codec.decode_stream(2), gt, schedule("ragged", gt.shape[1])).cpu().numpy()
    err = rms(rec.reshape(-1)[::REC_STRIDE] - z[f"{name}.rec_strided"])
    parity_record.record("encodec_dstream", f"{name}/ragged/fp32_exact", waveform_rms_err=err)
    print(f"encodec_dstream {name}/ragged fp32_exact: waveform RMS error {err:.3e}")
    assert err < WAVE_BAR, err


def test_tiny_config_streams(codecs, checkpoints):
    """The tiny architecture (LSTM width 64, 4 .. 64 channels).  Its fixtures are 3 frames long, shorter than the warm-up: seeded noise
    against the CPU oracle instead (fp32 one-shot tokens and waveform, fp64 margins)."""
    from oracle import encodec_oracle as O

    cfg, sd = checkpoints("tiny", 0)
    codec = codecs("tiny", 0)
    sig = noise(610, 2, 30 * HOP)
    W = O.fold_weight_norm(sd)
    with torch.no_grad():
        _, m64 = O.sig_to_toks(cfg, O.fold_weight_norm(sd, torch.float64), sig.double(), None, 8, True)
        otoks = O.sig_to_toks(cfg, W, sig)
        orec = O.toks_to_sig(cfg, W, otoks).numpy()
    toks = run_encode(codec.encode_stream(2), sig.cuda(), [n * HOP for n in schedule("ragged", 30)])
    check_tokens("tiny_noise/ragged", toks, otoks.numpy(), m64.numpy())
    rec = run_decode(codec.decode_stream(2), otoks.cuda(), schedule("one_frame", 30)).cpu().numpy()
    err = rms(rec - orec)
    print(f"encodec_dstream tiny_noise/one_frame: waveform RMS error {err:.3e}")
    assert err < WAVE_BAR, err


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------
def test_python_errors(codecs, checkpoints):
    from audiocodecs_amd import Encodec, EncodecDecodeStream, EncodecEncodeStream

    cfg, sd = checkpoints("tiny", 0)
    with pytest.raises(ValueError, match="decode"):
        Encodec(24000, mode="decode", state_dict=sd, config=cfg).encode_stream(1)
    with pytest.raises(ValueError, match="encode"):
        Encodec(24000, mode="encode", state_dict=sd, config=cfg).decode_stream(1)
    for fn in ("encode_stream", "decode_stream"):
        with pytest.raises(ValueError, match="resampling"):
            getattr(Encodec(16000, state_dict=sd, config=cfg), fn)(1)
        with pytest.raises(ValueError, match="bandwidth"):
            getattr(Encodec(24000, num_codebooks=3, state_dict=sd, config=cfg), fn)(1)
    codec = codecs("tiny")
    for bad in (0, -2, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            codec.encode_stream(bad)
        with pytest.raises(ValueError):
            codec.decode_stream(bad)
    s, d = codec.encode_stream(2), codec.decode_stream(2)
    assert isinstance(s, EncodecEncodeStream) and isinstance(d, EncodecDecodeStream)
    assert s.WARMUP_FRAMES == d.WARMUP_FRAMES == max(cfg.kernel_size, cfg.last_kernel_size)
    x = noise(611, 2, 9 * HOP).cuda()
    for bad in (x[:1], x[0], x.double(), x.long(), x.cpu(), x[:, None]):
        with pytest.raises(ValueError):
            s.push(bad)
    t = rand_toks(612, 2, 9)
    for bad in (t[:1], t[0], t.int(), t.float(), t.cpu(), t[:, :, :4], t[:, None]):
        with pytest.raises(ValueError):
            d.push(bad)
    assert s.push(x[:, :0]).shape == (2, 0, 8) and d.push(t[:, :0]).shape == (2, 0)
    assert torch.equal(s.push(x), codec.encode_stream(2).push(x))          # the streams still work after every refusal
    assert torch.equal(d.push(t), codec.decode_stream(2).push(t))


def test_abi_errors_leave_the_handle_usable(codecs, mimi_checkpoints):
    from audiocodecs_amd import Mimi
    from audiocodecs_amd.encodec import _ptr, _stream

    codec = codecs("tiny")
    B, F, K = 2, WARMUP, codec.num_codebooks
    x, sg = rand_toks(613, B, F), noise(614, B, F * HOP).cuda()
    keepd, keepe = codec.decode_stream(B), codec.encode_stream(B)     # (kept alive: the handle knows reset states by address)
    want_sig, want_toks = keepd.push(x), keepe.push(sg)
    nat = codec._native_for(x)
    L, h = nat.lib, nat.h
    db, eb = L.ac_encodec_stream_decode_state_bytes(h, B), L.ac_encodec_stream_state_bytes(h, B)
    dws, ews = L.ac_encodec_stream_decode_workspace_bytes(h, B, F), L.ac_encodec_stream_workspace_bytes(h, B, F)
    assert db > 0 and eb > 0 and dws > 0 and ews > 0
    big = max(db, eb)
    dstate = torch.empty(big, dtype=torch.uint8, device=x.device)
    estate = torch.empty(big, dtype=torch.uint8, device=x.device)
    ws = torch.empty(max(dws, ews), dtype=torch.uint8, device=x.device)
    sig = torch.empty(B, F * HOP, dtype=torch.float32, device=x.device)
    toks = torch.empty(B, F, K, dtype=torch.int64, device=x.device)

    def dec(st=dstate, sb=db, b=B, f=F, wb=dws, lib=L, hh=h):
        return lib.ac_encodec_stream_decode(hh, _ptr(st), sb, _ptr(x), b, f, K, _ptr(sig), _ptr(ws), wb, _stream())

    def enc(st=estate, sb=eb, b=B, f=F, wb=ews, lib=L, hh=h):
        return lib.ac_encodec_stream_encode(hh, _ptr(st), sb, _ptr(sg), b, f, K, _ptr(toks), _ptr(ws), wb, _stream())

    assert dec() == AC_EINVAL and enc() == AC_EINVAL                        # never reset
    mask = torch.ones(B, dtype=torch.uint8, device=x.device)
    assert L.ac_encodec_stream_decode_reset(h, _ptr(dstate), db, B, _ptr(mask), _stream()) == AC_EINVAL      # streams reset together
    assert L.ac_encodec_stream_decode_reset(h, _ptr(dstate), db - 256, B, None, _stream()) == AC_ENOMEM
    assert L.ac_encodec_stream_reset(h, _ptr(estate), eb - 256, B, None, _stream()) == AC_ENOMEM
    assert L.ac_encodec_stream_decode_reset(h, _ptr(dstate), db, B, None, _stream()) == 0
    assert L.ac_encodec_stream_reset(h, _ptr(estate), eb, B, None, _stream()) == 0
    assert dec(sb=db - 256) == AC_ENOMEM and enc(sb=eb - 256) == AC_ENOMEM   # state too small
    assert dec(wb=dws - 4096) == AC_ENOMEM and enc(wb=ews - 4096) == AC_ENOMEM   # workspace too small
    assert dec(b=1) == AC_EINVAL and enc(b=1) == AC_EINVAL                  # reset for another B
    assert dec(f=WARMUP - 1) == AC_EINVAL and enc(f=WARMUP - 1) == AC_EINVAL     # a fresh state needs the warm-up frames
    onat = codecs("tiny", 1)._native_for(x)                                 # another handle: never reset there
    assert dec(lib=onat.lib, hh=onat.h) == AC_EINVAL and enc(lib=onat.lib, hh=onat.h) == AC_EINVAL
    assert dec(st=estate, sb=big) == AC_EINVAL and enc(st=dstate, sb=big) == AC_EINVAL     # each kind where the other is expected
    assert dec() == 0 and enc() == 0
    torch.cuda.synchronize()
    assert torch.equal(sig, want_sig) and torch.equal(toks, want_toks)      # the refusals changed nothing
    x1 = x[:, :1].contiguous()
    sig1 = torch.empty(B, HOP, dtype=torch.float32, device=x.device)
    assert L.ac_encodec_stream_decode(h, _ptr(dstate), db, _ptr(x1), B, 1, K, _ptr(sig1), _ptr(ws), dws, _stream()) == 0   # F = 1 once warm
    assert torch.equal(sig1, keepd.push(x1))
    # a non-EnCodec handle
    mcfg, msd = mimi_checkpoints("tiny", 0)
    m = Mimi(24000, state_dict=msd, config=mcfg)
    mnat = m._native_for(x)
    for fn in (L.ac_encodec_stream_state_bytes, L.ac_encodec_stream_decode_state_bytes):
        assert fn(mnat.h, B) == 0
    for fn in (L.ac_encodec_stream_workspace_bytes, L.ac_encodec_stream_decode_workspace_bytes):
        assert fn(mnat.h, B, F) == 0
    assert L.ac_encodec_stream_reset(mnat.h, _ptr(estate), eb, B, None, _stream()) == AC_EINVAL
    assert L.ac_encodec_stream_decode_reset(mnat.h, _ptr(dstate), db, B, None, _stream()) == AC_EINVAL
    assert codec.decode_stream(B).push(x).equal(want_sig)
