"""GPU parity: the HIP path (through the C ABI, via audiocodecs_amd.Encodec) against
(a) the reference-generated golden fixtures and (b) the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): token ids bit-exact, waveform within 1e-4 RMS.  fp32 summation
order differs between any two implementations (the reference itself flips 0.008 % of tokens
between 1 and 8 CPU threads), so token equality is REQUIRED wherever the fp64
margin between best and second-best codeword exceeds TAU at this and all earlier stages of the
frame, and the remainder is counted and bounded, not hidden.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from golden_cases import CASES, REC_STRIDE, make_input, noise
from test_oracle_golden import TAU, tokens_match_up_to_ties
import layer_cases as LC
import parity_record

pytestmark = pytest.mark.gpu

ENC_TAPS = ["enc0", "enc1", "enc3", "enc4", "enc6", "enc7", "enc9", "enc10", "enc12", "enc13"]
DEC_TAPS = ["dec0", "dec1", "dec3", "dec4", "dec6", "dec7", "dec9", "dec10", "dec12", "dec13"]


@pytest.fixture(scope="module")
def codecs(checkpoints):
    from audiocodecs_amd import Encodec

    cache = {}

    def get(cfg_name, seed, K=8):
        key = (cfg_name, seed, K)
        if key not in cache:
            cfg, sd = checkpoints(cfg_name, seed)
            cache[key] = Encodec(24000, num_codebooks=K, state_dict=sd, config=cfg).eval()
        return cache[key]

    return get


def rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


def capture(codec, fn, nfloats=1 << 24):
    nat = next(iter(codec._natives.values()))
    buf = torch.zeros(nfloats, device="cuda")
    nat.lib.ac_debug_capture(nat.h, C.c_void_p(buf.data_ptr()), nfloats)
    try:
        out = fn()
        torch.cuda.synchronize()
        used = nat.lib.ac_debug_captured(nat.h)
    finally:
        nat.lib.ac_debug_capture(nat.h, None, 0)
    assert used <= nfloats
    return out, buf[:used].cpu().numpy()


@pytest.mark.parametrize("name", ["tiny_taps", "tiny_ragged"])
def test_every_module_output_matches_reference_hooks(name, golden, codecs):
    """Tiny architecture: each module output of the HIP path vs the reference's forward hooks."""
    z, meta = golden
    case = next(c for c in CASES if c["name"] == name)
    codec = codecs("tiny", 0)
    inp = make_input(case, GOLDEN_DIR)
    sig = inp["sig"].cuda()
    length = inp["length"].cuda() if "length" in inp else None
    codec.sig_to_toks(sig[:, :64])  # creates the native handle
    toks, flat = capture(codec, lambda: codec.sig_to_toks(sig, length))
    off = 0
    for tap in ENC_TAPS:
        g = z[f"{name}.act.{tap}"]  # [B,C,L]
        n = g.size
        got = flat[off : off + n].reshape(g.shape[0], g.shape[2], g.shape[1]).transpose(0, 2, 1)
        np.testing.assert_allclose(got, g, atol=3e-6, rtol=1e-5, err_msg=tap)
        off += n
    assert off == flat.size
    gold = z[f"{name}.toks"].astype(np.int64)
    assert np.array_equal(toks.cpu().numpy(), gold)  # min margin of these fixtures is > 2e-3
    gt = torch.from_numpy(gold).cuda()
    rec, flat = capture(codec, lambda: codec.toks_to_sig(gt))
    off = 0
    for tap in DEC_TAPS:
        g = z[f"{name}.act.{tap}"]
        n = g.size
        got = flat[off : off + n].reshape(g.shape[0], g.shape[2], g.shape[1]).transpose(0, 2, 1)
        np.testing.assert_allclose(got, g, atol=5e-6, rtol=1e-5, err_msg=tap)
        off += n
    np.testing.assert_allclose(rec.cpu().numpy(), z[f"{name}.rec_full"], atol=5e-6)
    feats = codec.sig_to_feats(sig, length)
    np.testing.assert_allclose(feats.cpu().numpy(), z[f"{name}.feats"], atol=5e-6)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_golden_fixture(case, golden, codecs):
    z, meta = golden
    name = case["name"]
    info = meta["cases"][name]
    codec = codecs(case["cfg"], case["weights_seed"], info["K"])
    inp = make_input(case, GOLDEN_DIR)
    if case["kind"] == "decode":
        toks = inp["toks"].cuda()
    else:
        sig = inp["sig"].cuda()
        length = inp["length"].cuda() if "length" in inp else None
        toks = codec.sig_to_toks(sig, length)
        assert toks.dtype == torch.int64 and list(toks.shape) == info["toks_shape"]
        gold = z[f"{name}.toks"].astype(np.int64)
        margin = z[f"{name}.margin64"]
        mism, bad, excused = parity_record.tokens("encodec", name, toks.cpu().numpy(), gold, margin, TAU)
        assert bad == 0, f"{bad} tokens differ outside near-ties"
        if margin.min() > TAU:       # no near-tie anywhere in the fixture: bit-exact, nothing to excuse
            assert np.array_equal(toks.cpu().numpy(), gold)
        assert mism <= excused       # a difference can only sit in a frame that had an fp64 near-tie
        feats = codec.sig_to_feats(sig, length).cpu().numpy()
        err = feats.reshape(-1)[::REC_STRIDE] - z[f"{name}.feats_strided"]
        assert rms(err) < 2e-5 and np.abs(err).max() < 2e-4
        parity_record.record("encodec", name, feats_rms_err=rms(err))
        toks = torch.from_numpy(gold).cuda()  # decode the REFERENCE's tokens
    rec = codec.toks_to_sig(toks).cpu().numpy()
    assert list(rec.shape) == info["rec_shape"]
    err = rec.reshape(-1)[::REC_STRIDE] - z[f"{name}.rec_strided"]
    parity_record.record("encodec", name, waveform_rms_err=rms(err))
    assert rms(err) < 1e-4, rms(err)          # the north-star bar
    assert rms(err) < 1e-5, rms(err)          # what fp32 parity mode actually delivers
    assert abs(rms(rec) - info["rec_rms"]) < 1e-4


def test_against_oracle_on_fresh_inputs(codecs, checkpoints):
    """Seeded inputs that are in no fixture: HIP vs the CPU oracle (fp32) with fp64 margins."""
    from oracle import encodec_oracle as O

    cfg, sd = checkpoints("full", 0)
    codec = codecs("full", 0)
    W = O.fold_weight_norm(sd)
    W64 = O.fold_weight_norm(sd, torch.float64)
    sig = noise(977, 3, 36001)
    length = torch.tensor([1.0, 0.83, 0.5])
    with torch.no_grad():
        otoks = O.sig_to_toks(cfg, W, sig, length)
        _, m64 = O.sig_to_toks(cfg, W64, sig.double(), length.double(), 8, True)
        orec = O.toks_to_sig(cfg, W, otoks)
    toks = codec.sig_to_toks(sig.cuda(), length.cuda())
    mism, bad, excused = parity_record.tokens("encodec", "oracle_fresh_b3", toks.cpu().numpy(), otoks.numpy(), m64.numpy(), TAU)
    assert bad == 0 and mism <= excused
    rec = codec.toks_to_sig(otoks.cuda()).cpu()
    parity_record.record("encodec", "oracle_fresh_b3", waveform_rms_err=rms((rec - orec).numpy()))
    assert rms((rec - orec).numpy()) < 1e-5
    # reconstruct mode == sig_to_toks then toks_to_sig (codec.py:45-55)
    rec2 = codec(sig.cuda(), length.cuda())
    assert torch.equal(rec2, codec.toks_to_sig(toks))


@pytest.mark.parametrize("B,T", [(33, 6400), (1, 48000), (5, 3333)])
def test_odd_batches_against_oracle(B, T, codecs, checkpoints):
    """Batch sizes that leave the 32-clip LSTM tile / 16-frame RVQ tile partially filled."""
    from oracle import encodec_oracle as O

    cfg, sd = checkpoints("full", 0)
    codec = codecs("full", 0)
    W = O.fold_weight_norm(sd)
    W64 = O.fold_weight_norm(sd, torch.float64)
    sig = noise(1000 + B, B, T)
    with torch.no_grad():
        otoks = O.sig_to_toks(cfg, W, sig)
        _, m64 = O.sig_to_toks(cfg, W64, sig.double(), None, 8, True)
        orec = O.toks_to_sig(cfg, W, otoks)
    toks = codec.sig_to_toks(sig.cuda())
    mism, bad, excused = parity_record.tokens("encodec", f"oracle_B{B}_T{T}", toks.cpu().numpy(), otoks.numpy(), m64.numpy(), TAU)
    assert bad == 0 and mism <= excused
    rec = codec.toks_to_sig(otoks.cuda()).cpu()
    parity_record.record("encodec", f"oracle_B{B}_T{T}", waveform_rms_err=rms((rec - orec).numpy()))
    assert rms((rec - orec).numpy()) < 1e-5


@pytest.mark.parametrize("B,T", [(80, 24000), (130, 9600)])
def test_batches_beyond_one_lstm_launch(B, T, codecs):
    """More than 64 clips: the persistent LSTM runs once per 64-clip chunk (the self-validating h buffers are re-filled
    before every launch); clips are independent units, so any split of the batch gives the same ids and samples."""
    codec = codecs("full", 0)
    sig = noise(2000 + B, B, T).cuda()
    toks = codec.sig_to_toks(sig)
    parts = torch.cat([codec.sig_to_toks(sig[i : i + 16]) for i in range(0, B, 16)])
    assert torch.equal(toks, parts)
    rec = codec.toks_to_sig(toks)
    recp = torch.cat([codec.toks_to_sig(toks[i : i + 16]) for i in range(0, B, 16)])
    assert torch.equal(rec, recp)


def test_rest_of_codec_api(codecs, checkpoints):
    from oracle import encodec_oracle as O

    cfg, sd = checkpoints("full", 0)
    codec = codecs("full", 0)
    W = O.fold_weight_norm(sd)
    toks = torch.from_numpy(make_input(next(c for c in CASES if c["name"] == "full_decode_rand"), GOLDEN_DIR)["toks"].numpy())
    q = codec.toks_to_qfeats(toks.cuda()).cpu()
    with torch.no_grad():
        oq = O.toks_to_qfeats(cfg, W, toks)
    np.testing.assert_allclose(q.numpy(), oq.numpy(), atol=1e-6)
    e = codec.embs().cpu()
    assert e.shape == (8, 1024, 128) and torch.equal(e, O.embs(W, 8))
    sig = noise(5, 2, 4000).cuda()
    qf = codec.sig_to_qfeats(sig)
    assert torch.equal(qf, codec.toks_to_qfeats(codec.sig_to_toks(sig)))
    lg = codec.logits()
    assert lg.shape == (8, 1024, 1024)
    r = codec.resample(codec.sig_to_toks(sig), p=0.5)
    assert r.shape == (2, 13, 8) and int(r.max()) < 1024


def test_error_behaviour(codecs, checkpoints):
    from audiocodecs_amd import Encodec
    from audiocodecs_amd._native import NativeError, debug_set

    cfg, sd = checkpoints("tiny", 0)
    with pytest.raises(ValueError):
        Encodec(24000, mode="bogus", state_dict=sd, config=cfg)
    c3 = Encodec(24000, num_codebooks=3, state_dict=sd, config=cfg)
    with pytest.raises(ValueError):  # [HF]:564-567: 2.25 kbps is not a target bandwidth
        c3.sig_to_toks(torch.zeros(1, 100, device="cuda"))
    c8 = codecs("tiny", 0)
    with pytest.raises(RuntimeError):  # relative lengths must peak at 1.0 (mask/signal shape mismatch upstream)
        c8.sig_to_toks(torch.zeros(2, 100, device="cuda"), torch.tensor([0.5, 0.25], device="cuda"))
    with pytest.raises(NativeError):
        c8.sig_to_toks(torch.zeros(1, 100))  # CPU tensor: no fallback
    with pytest.raises(NativeError):
        c8.toks_to_sig(torch.zeros(1, 3, 33, dtype=torch.long, device="cuda"))  # K > num_quantizers


def test_persistent_and_per_step_lstm_agree(checkpoints, monkeypatch):
    """The single-launch LSTM (lstm_persist.h; full-width model on a 256-CU device) and the per-step fallback
    (AC_LSTM=step, also what narrower models use) are the same function up to fp32 summation order."""
    from audiocodecs_amd import Encodec

    cfg, sd = checkpoints("full", 0)
    sig = noise(4242, 5, 16000).cuda()          # 5 clips: a partial 16-clip group
    fast = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    a = fast.sig_to_feats(sig)
    nat = next(iter(fast._natives.values()))
    assert nat.lib.ac_lstm_status(nat.h) == 1   # persistent path in use, no timeout
    monkeypatch.setenv("AC_LSTM", "step")
    slow = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    b = slow.sig_to_feats(sig)
    nat2 = next(iter(slow._natives.values()))
    assert nat2.lib.ac_lstm_status(nat2.h) == 0
    assert rms((a - b).cpu().numpy()) < 2e-6
    ra, rb = fast.toks_to_sig(fast.sig_to_toks(sig)), slow.toks_to_sig(fast.sig_to_toks(sig))
    assert rms((ra - rb).cpu().numpy()) < 2e-6
    big = noise(4243, 70, 3200).cuda()          # 70 clips: two cooperative launches (64 + 6)
    assert rms((fast.sig_to_feats(big) - slow.sig_to_feats(big)).cpu().numpy()) < 2e-6


def test_split_operand_and_exact_product_kernels_agree(checkpoints, golden, monkeypatch):
    """Default: GEMMs / LSTM products in split16 arithmetic on the fp16 pipe (tap_gemm6.h, lstm_persist16.h).
    AC_GEMM=fp32: exact fp32 products (tap_gemm4.h, lstm_persist.h).  Same function up to fp32-level rounding, and the
    exact-product build also reproduces the reference's tokens."""
    from audiocodecs_amd import Encodec

    z, meta = golden
    cfg, sd = checkpoints("full", 0)
    sig = noise(5151, 3, 24000).cuda()
    fast = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    fa, ta = fast.sig_to_feats(sig), fast.sig_to_toks(sig)
    monkeypatch.setenv("AC_GEMM", "fp32")
    exact = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    fb, tb = exact.sig_to_feats(sig), exact.sig_to_toks(sig)
    assert rms((fa - fb).cpu().numpy()) < 3e-6
    assert float((ta == tb).float().mean()) > 0.999   # two fp32-faithful arithmetics: only fp32-level near-ties may differ
    assert rms((fast.toks_to_sig(ta) - exact.toks_to_sig(ta)).cpu().numpy()) < 3e-6
    case = next(c for c in CASES if c["name"] == "full_noise_b2")
    inp = make_input(case, GOLDEN_DIR)
    toks = exact.sig_to_toks(inp["sig"].cuda())
    n, bad, excused = tokens_match_up_to_ties(toks.cpu().numpy(), z["full_noise_b2.toks"].astype(np.int64), z["full_noise_b2.margin64"])
    assert bad == 0


def _full_taps(direction):
    from audiocodecs_amd.config import ENCODEC_24KHZ

    return [t.name for t in LC.taps_of("encodec", ENCODEC_24KHZ, direction)]


FULL_ENC_TAPS = _full_taps("encode")     # (tests/test_fused_chains_gpu.py reads these)
FULL_DEC_TAPS = _full_taps("decode")


def test_every_module_output_full_config_production_kernels(codecs, checkpoints):
    """FULL architecture through the production kernels: enc_stream (stem, first residual block and first down-sampler as one
    chain), rb_stream6 / rb_stream128m (the 64- and 128-channel residual blocks), rb_fused6 (the 256-channel one), the tap-GEMMs,
    the persistent LSTM (lstm_persist16) and dec_stream (last up-sampler, last residual block and head).  Arming the capture hook
    does not change kernel selection on this path -- the chains write their inner module outputs themselves while it is armed
    (tests/test_layer_isolation_gpu.py::test_production_kernels_run_under_the_hook pins the names).  Every module output of a 1 s
    clip against the oracle's taps (the oracle is pinned to the reference's hooks on the tiny config and to its end-to-end outputs on
    this one); the tap order comes from tests/layer_cases.py.  A localized error shows up at its layer, not as a vague feature RMS."""
    from oracle import encodec_oracle as O

    cfg, sd = checkpoints("full", 0)
    codec = codecs("full", 0)
    W = O.fold_weight_norm(sd)
    sig = noise(8080, 2, 24000)
    taps, dtaps = {}, {}
    with torch.no_grad():
        O.masked_embeddings(cfg, W, sig, None, taps=taps)
        otoks = O.sig_to_toks(cfg, W, sig)
        orec = O.toks_to_sig(cfg, W, otoks, taps=dtaps)
    codec.sig_to_toks(sig[:, :640].cuda())
    nat = next(iter(codec._natives.values()))
    assert nat.lib.ac_lstm_status(nat.h) == 1   # the persistent LSTM is what runs
    _, flat = capture(codec, lambda: codec.sig_to_toks(sig.cuda()), 1 << 26)
    worst = {}
    enc = LC.taps_of("encodec", cfg, "encode")
    got_of = LC.split_capture(flat, enc, lambda t: taps[t.name].shape)
    for tap in (t.name for t in enc):
        g, got = taps[tap].numpy(), got_of[tap]  # [B,C,L]
        worst[tap] = float(np.abs(got - g).max() / max(1e-30, np.abs(g).max()))
        np.testing.assert_allclose(got, g, atol=5e-6 * max(1.0, float(np.abs(g).max())), rtol=2e-5, err_msg=tap)
    rec, flat = capture(codec, lambda: codec.toks_to_sig(otoks.cuda()), 1 << 26)
    dec = LC.taps_of("encodec", cfg, "decode")
    got_of = LC.split_capture(flat, dec, lambda t: dtaps[t.name].shape)
    for tap in (t.name for t in dec):
        g, got = dtaps[tap].numpy(), got_of[tap]
        worst[tap] = float(np.abs(got - g).max() / max(1e-30, np.abs(g).max()))
        np.testing.assert_allclose(got, g, atol=5e-6 * max(1.0, float(np.abs(g).max())), rtol=2e-5, err_msg=tap)
    parity_record.record("encodec", "full_config_module_taps", worst_rel_err_per_tap=worst,
                         waveform_rms_err=rms((rec.cpu() - orec).numpy()))
    assert rms((rec.cpu() - orec).numpy()) < 1e-5


def test_nan_clip_does_not_stall_or_poison_other_clips(codecs):
    """One clip with a NaN sample in a batch of 4: the call takes its normal time, the other three clips are bit-identical
    to a clean run, the NaN clip's LSTM output is NaN from the poisoned frame on (as the reference's LSTM gives), and the
    persistent kernel's status stays clean (lstm_persist6.h publish step + lstm_tail_kernel)."""
    import time

    codec = codecs("full", 0)
    sig = noise(9191, 4, 48000).cuda()
    clean_t = codec.sig_to_toks(sig)
    clean_f = codec.sig_to_feats(sig)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    codec.sig_to_feats(sig)
    torch.cuda.synchronize()
    t_clean = time.perf_counter() - t0
    bad = sig.clone()
    bad[2, 20000] = float("nan")
    t0 = time.perf_counter()
    f = codec.sig_to_feats(bad)
    torch.cuda.synchronize()
    t_bad = time.perf_counter() - t0
    assert t_bad < 5 * t_clean + 0.05, (t_bad, t_clean)   # a stalled exchange would spin for ~0.5 s per step
    toks = codec.sig_to_toks(bad)
    for b in (0, 1, 3):
        assert torch.equal(f[b], clean_f[b]) and torch.equal(toks[b], clean_t[b])
    frame = 20000 // 320
    assert torch.equal(f[2, : frame - 1], clean_f[2, : frame - 1])   # causal: frames before the NaN sample's receptive field
    assert bool(torch.isnan(f[2, frame + 1 :]).all())                # ... and NaN ever after (the LSTM carries it forward)
    assert bool((toks[2, frame + 1 :] == 0).all())                   # torch's argmax over an all-NaN row: index 0
    nat = next(iter(codec._natives.values()))
    assert nat.lib.ac_lstm_status(nat.h) == 1
    assert torch.equal(codec.sig_to_toks(sig), clean_t)              # and the handle is as good as before


def test_out_of_range_token_ids_are_reported(codecs):
    """F.embedding raises on an id outside the codebook.  No entry point synchronises, so the decode kernel sets the
    frame to NaN and the NEXT call on the handle fails with AC_EINVAL (once); afterwards the handle works again."""
    from audiocodecs_amd._native import NativeError, debug_set

    codec = codecs("full", 0)
    toks = torch.randint(0, 1024, (2, 6, 8), device="cuda")
    good = codec.toks_to_qfeats(toks)
    toks2 = toks.clone()
    toks2[1, 3, 5] = 1024
    q = codec.toks_to_qfeats(toks2)
    torch.cuda.synchronize()
    assert bool(torch.isnan(q[1, 3]).all()) and torch.equal(q[0], good[0]) and torch.equal(q[1, :3], good[1, :3])
    with pytest.raises(NativeError, match="token ids outside"):
        codec.toks_to_qfeats(toks)
    assert torch.equal(codec.toks_to_qfeats(toks), good)


def test_mode_drops_the_unused_half(checkpoints):
    """encodec.py:67-71: mode="encode" deletes the decoder, mode="decode" the encoder.  Here the unused half is never
    packed or uploaded; calling it reports the missing half instead of running on absent weights."""
    from audiocodecs_amd import Encodec
    from audiocodecs_amd._native import NativeError, debug_set

    cfg, sd = checkpoints("full", 0)
    both = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    enc = Encodec(24000, mode="encode", num_codebooks=8, state_dict=sd, config=cfg).eval()
    dec = Encodec(24000, mode="decode", num_codebooks=8, state_dict=sd, config=cfg).eval()
    sig = noise(6161, 2, 8000).cuda()
    toks = both.sig_to_toks(sig)
    assert torch.equal(enc(sig), toks)                       # forward() in encode mode = sig_to_toks (codec.py:45-55)
    assert torch.equal(dec(toks), both.toks_to_sig(toks))
    with pytest.raises(NativeError, match="without decoder weights"):
        enc.toks_to_sig(toks)
    with pytest.raises(NativeError, match="without encoder weights"):
        dec.sig_to_toks(sig)
