"""The 16 kHz and 24 kHz DAC models (config.DAC_16KHZ, 12 codebooks; config.DAC_24KHZ, 32) at FULL width on the GPU.

`audiocodecs_amd.DAC` picks its model from `orig_sample_rate` as the reference wrapper does, and the default is the 16 kHz one.
Both differ from the 44.1 kHz model, the one every other DAC test builds, where kernels are chosen:

  * strides (2,4,5,8): the x5 conv (256 -> 512, k10, K = 2560, segment row 5 x 256) and the x5 transposed conv (768 -> 384 as a
    tap-GEMM of N = 5 x 384 = 1920 columns with y_off = -3 x 384 and y_len trimming both ends).  1920 is a multiple of 128 and not
    of 256, which no transposed conv of the 44.1 kHz model is: the trimmed store of the 128-column arrangements runs here only.
    (DAC_TINY has the odd stride too, at N = 80: exact-fp32 tap_gemm4 products only.)
  * 12 and 32 codebooks: dac_vq_encode_kernel keeps its residual tile in LDS through all stages; ac_embs, ac_embs_projected,
    rvq_decode_kernel and the workspace sizes had not seen more than 9.

The tests: the stand-in fixtures of tests/golden/dac_rates_golden.npz (test_golden_fixture, the bars of tests/test_dac_gpu_parity.py),
the CPU oracle on fresh inputs at (2, 2049) and (3, 10891) -- 34 frames, a ragged last hop, the x5 conv writes 272 rows and the x5
transposed conv reads 272: 128- and 256-row tiles both have a seam and a partial last tile -- every layer alone against fp64
(tests/test_layer_isolation_gpu.py's `isolate` and bar), the kernels the two stride-5 layers ran as, batch independence across
two routes, the wrapper as the reference calls it, and a bad token id in the last of 32 codebooks."""
import math
import re

import numpy as np
import pytest
import torch

import layer_cases as LC
import parity_record
from conftest import GOLDEN_DIR
from dac_cases import RATE_CASES, rate_checkpoint
from golden_cases import noise
from test_dac_gpu_parity import check_golden_case
from test_gpu_parity import capture, rms
from test_layer_isolation_gpu import _captured_decode, isolate
from test_oracle_golden import TAU, tokens_match_up_to_ties

pytestmark = pytest.mark.gpu

TAGS = ["dac16", "dac24"]
FRESH = [(2, 2049), (3, 10891)]
_CACHE = {}


def _oracle():
    from oracle import dac_oracle as O

    return O


def _weights(tag):
    """-> (cfg, state dict, W fp32, W fp64), once per module."""
    if ("W", tag) not in _CACHE:
        cfg, sd = rate_checkpoint(tag)
        O = _oracle()
        _CACHE["W", tag] = (cfg, sd, O.cast_weights(sd), O.cast_weights(sd, torch.float64))
    return _CACHE["W", tag]


def _codec(tag, K=None, latent=False, precision=None):
    cfg, sd, _, _ = _weights(tag)
    K = cfg.n_codebooks if K is None else K
    key = ("codec", tag, K, latent, precision)
    if key not in _CACHE:
        from audiocodecs_amd import DAC

        c = DAC(cfg.sampling_rate, cfg.sampling_rate, num_codebooks=K, latent=latent, state_dict=sd, config=cfg, precision=precision).eval()
        # `num_codebooks` and `latent` are arguments of the calls, not of the handle: the wrappers of one (model, precision) share the
        # first one's handle instead of packing and uploading the 75 M weights once more each
        first = _CACHE.setdefault(("handle", tag, precision), c)
        c._natives = first._natives
        c.sig_to_feats(noise(1, 1, 640).cuda())          # creates the native handle
        _CACHE[key] = c
    return _CACHE[key]


@pytest.fixture(scope="module")
def rates_golden():
    import json
    import os

    z = np.load(os.path.join(GOLDEN_DIR, "dac_rates_golden.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


# ------------------------------------------------------------------------------------------------ a. the stand-in fixtures
@pytest.mark.parametrize("case", RATE_CASES, ids=[c["name"] for c in RATE_CASES])
def test_golden_fixture(case, rates_golden):
    """tests/test_dac_gpu_parity.py::test_golden_fixture on the new cases, its bars unchanged: tokens exact outside fp64 near-ties,
    feats rms < 3e-5 and max < 5e-4, latent and qfeats atol 5e-5, waveform rms < 3e-5, embs atol 3e-6."""
    z, meta = rates_golden
    check_golden_case(case, z, meta, lambda tag, seed, K, latent=False: _codec(tag, K, latent))


@pytest.mark.parametrize("tag", TAGS)
def test_embs_whole_tables_against_the_oracle(tag):
    """The fixture file holds every 4999th entry of the tables; here all of ac_embs / ac_embs_projected at K = 12 and K = 32 against
    the oracle (which the CPU test pins to the same fixture), under the fixture's bar."""
    cfg, sd, W, _ = _weights(tag)
    O = _oracle()
    for latent in (True, False):
        e = _codec(tag, latent=latent).embs()
        with torch.no_grad():
            ref = O.embs(cfg, W, cfg.n_codebooks, latent)
        assert tuple(e.shape) == tuple(ref.shape) == (cfg.n_codebooks, 1024, cfg.codebook_dim if latent else cfg.hidden_size)
        np.testing.assert_allclose(e.cpu().numpy(), ref.numpy(), rtol=0, atol=3e-6)


# ------------------------------------------------------------------------------------------------ b. the oracle on fresh inputs
def _fresh(tag, B, T):
    """Signal and the oracle's outputs for it (fp32 tokens, features, waveform; fp64 margins), once per module."""
    key = ("fresh", tag, B, T)
    if key not in _CACHE:
        cfg, sd, W, W64 = _weights(tag)
        O, K = _oracle(), cfg.n_codebooks
        torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
        sig = noise(9400 + T + cfg.sampling_rate // 1000, B, T)
        with torch.no_grad():
            otoks = O.sig_to_toks(cfg, W, sig, None, K)
            _, m64 = O.sig_to_toks(cfg, W64, sig.double(), None, K, "descript", True)
            orec = O.toks_to_sig(cfg, W, otoks)
            ofeats = O.sig_to_feats(cfg, W, sig)
        _CACHE[key] = (sig, otoks, m64.numpy(), orec, ofeats)
    return _CACHE[key]


@pytest.mark.parametrize("B,T", FRESH)
@pytest.mark.parametrize("tag", TAGS)
def test_against_oracle_on_fresh_inputs(tag, B, T):
    """The bars of tests/test_dac_gpu_parity.py::test_against_oracle_on_fresh_inputs, all codebooks.  The near-tie excuse is bounded
    BEFORE the device is called, from the fp64 margins alone: at most 5 % of the tokens excused, at least 90 % of the frames still
    judged at the last stage (the reference alone: 0 % excused on both 16 kHz cases; 0 % and 0.8 % at 24 kHz, 99 % of the frames
    of (3, 10891) judged at stage 32)."""
    cfg, sd, W, W64 = _weights(tag)
    K = cfg.n_codebooks
    sig, otoks, m64, orec, ofeats = _fresh(tag, B, T)
    assert tuple(otoks.shape) == (B, cfg.num_frames(T), K)
    safe = np.cumprod(m64 > TAU, axis=-1).astype(bool)
    excused, judged_last = float((~safe).mean()), float(safe[..., -1].mean())
    print(f"{tag} ({B}, {T}): {100 * excused:.2f} % of the tokens excused, {100 * judged_last:.1f} % of the frames judged at stage {K}")
    assert excused <= 0.05 and judged_last >= 0.90, (excused, judged_last)
    codec = _codec(tag)
    toks = codec.sig_to_toks(sig.cuda())
    assert toks.dtype == torch.int64 and tuple(toks.shape) == tuple(otoks.shape)
    mism, bad, n_excused = parity_record.tokens(tag, f"fresh_B{B}_T{T}", toks.cpu().numpy(), otoks.numpy(), m64, TAU)
    n, bad2, _ = tokens_match_up_to_ties(toks.cpu().numpy(), otoks.numpy(), m64)
    assert bad == bad2 == 0, f"{bad}/{n}"
    assert rms(codec.sig_to_feats(sig.cuda()).cpu().numpy() - ofeats.numpy()) < 3e-5
    rec = codec.toks_to_sig(otoks.cuda()).cpu().numpy()
    err = rms(rec - orec.numpy()) if rec.shape == tuple(orec.shape) else None
    parity_record.record(tag, f"fresh_B{B}_T{T}", waveform_rms_err=err)
    assert rec.shape == tuple(orec.shape) == (B, cfg.num_samples(cfg.num_frames(T))) and err < 3e-5, err
    out = codec(sig.cuda())  # Codec.forward, mode "reconstruct"
    assert out.shape == rec.shape


# ------------------------------------------------------------------------------------------------ c. every layer alone against fp64
ISO_SEEDS = {"dac16": 9316, "dac24": 9324}
STRIDE5 = {"encoder.block.2.conv1", "decoder.block.1.conv_t1"}                 # downsampling_ratios[2] == upsampling_ratios[1] == 5
STRIDE5_AND_NEIGHBOURS = STRIDE5 | {"encoder.block.2.res_unit3", "encoder.block.3.res_unit1", "decoder.block.0.res_unit3", "decoder.block.1.res_unit1"}


def _iso_signal(tag, which, B, T):
    return LC.gain_input(noise(ISO_SEEDS[tag], B, T), which, noise(ISO_SEEDS[tag] + 50, 1, 400)[0])


def _isolate_case(tag, precision, which, B, T, only=None):
    cfg, sd, W, W64 = _weights(tag)
    assert cfg.downsampling_ratios[2] == cfg.upsampling_ratios[1] == 5
    O = _oracle()
    codec = _codec(tag, precision=precision)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    case = f"{precision or 'split16'}/{which}" + ("" if only is None else f"/stride5_B{B}_T{T}")
    sig = _iso_signal(tag, which, B, T)
    _, flat = capture(codec, lambda: codec.sig_to_toks(sig.cuda()), 1 << 26)
    failures = isolate("dac", cfg, W, W64, "encode", flat, sig[:, None], case, only, record_as=tag)
    if ("isotoks", tag, which, B, T) not in _CACHE:      # decoding takes the fp32 oracle's tokens of the same signal (both precisions)
        with torch.no_grad():
            _CACHE["isotoks", tag, which, B, T] = O.sig_to_toks(cfg, W, sig, None, cfg.n_codebooks)
    toks = _CACHE["isotoks", tag, which, B, T]
    with torch.no_grad():
        x0 = O.from_codes(cfg, W, toks.movedim(-1, -2))[0]          # (the hook emits it as the first, skipped tap: only its shape is used)
    rec, flat = _captured_decode(codec, toks, fused_units=precision is None)
    assert bool(torch.isfinite(rec).all())
    failures += isolate("dac", cfg, W, W64, "decode", flat, x0, case, only, result=rec.cpu(), record_as=tag)
    return failures


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("precision", [None, "fp32_exact"], ids=["split16", "fp32_exact"])
@pytest.mark.parametrize("tag", TAGS)
def test_every_layer_alone_against_fp64(tag, precision, which):
    """tests/test_layer_isolation_gpu.py at (2, 2049) for both models: every layer from the GPU's own previous tap against fp64 under
    that file's elementwise bar; e_gpu, e_ref and worst_err_over_tol go to the parity record under dac16/... and dac24/... ."""
    failures = _isolate_case(tag, precision, which, 2, 2049)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("tag", TAGS)
def test_stride5_layers_alone_past_the_tile_seams(tag):
    """(3, 10891), split16: the x5 conv writes 272 rows per clip and the x5 transposed conv reads 272 (273 tap-GEMM rows, 1360 output
    rows trimmed at both ends) -- past one 256-row tile and two 128-row tiles, each with a partial last tile.  Only the two stride-5
    layers and the residual units on either side of them are recomputed; the other taps are walked over by size."""
    failures = _isolate_case(tag, None, "A", 3, 10891, only=lambda t: t.name in STRIDE5_AND_NEIGHBOURS)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ d. the routes that ran
ENC5 = re.compile(r"^(tap_gemm\w*_kernel<[^>]*>) B(\d+) M(\d+) N512 K2560 J2 s5$")          # 256 -> 512, k10: K = 10 x 256
DEC5 = re.compile(r"^(tap_gemm\w*_kernel<[^>]*>) B(\d+) M(\d+) N1920 K1536 J2 s1$")         # 768 -> 5 x 384 from [x[m-1] | x[m]]: K = 2 x 768

TINY8_128, TINY8_256 = "tap_gemm8_kernel<4, 2, 2, 2, 2>", "tap_gemm8_kernel<2, 4, 2, 2, 2>"   # the tiny-launch rule's tile forms
# (B, T) -> the profile records of the x5 conv and of the x5 transposed conv, split16 precision; the same for both models (the
# two layers have the same shapes).  From runs with "prof_detail" on.
ROUTES = {
    (1, 320):   (f"{TINY8_256} B1 M8 N512 K2560 J2 s5",   f"{TINY8_128} B1 M9 N1920 K1536 J2 s1"),
    (2, 2049):  (f"{TINY8_256} B2 M51 N512 K2560 J2 s5",  f"{TINY8_128} B2 M49 N1920 K1536 J2 s1"),
    (5, 2049):  (f"{TINY8_256} B5 M51 N512 K2560 J2 s5",  "tap_gemm6_kernel<1, 4, 4, 1, 2> B5 M49 N1920 K1536 J2 s1"),
    (3, 10891): (f"{TINY8_256} B3 M272 N512 K2560 J2 s5", "tap_gemm6_kernel<1, 4, 4, 1, 2> B3 M273 N1920 K1536 J2 s1"),
}


def _tiny_launch(rec):
    """csrc/tap_route.h: at most 64 tiles of 128 x 128 -> the tiny-launch rule decides, not the cost model."""
    m = ENC5.match(rec) or DEC5.match(rec)
    B, M, N = int(m.group(2)), int(m.group(3)), int(re.search(r" N(\d+) ", rec).group(1))
    return B * math.ceil(M / 128) * (N // 128) <= 64


def _stride5_records(codec, sig, toks=None):
    """(record of the x5 conv, record of the x5 transposed conv, tokens, waveform) of one encode + decode with "prof_detail" on."""
    from audiocodecs_amd._native import debug_set

    out = {}

    def run():
        out["toks"] = codec.sig_to_toks(sig)
        out["rec"] = codec.toks_to_sig(out["toks"] if toks is None else toks)

    debug_set(codec, "prof_detail", 1)
    try:
        names = [s[0] for s in codec.profile_kernels(run)]
    finally:
        debug_set(codec, "prof_detail", 0)
    enc, dec = [n for n in names if ENC5.match(n)], [n for n in names if DEC5.match(n)]
    assert len(enc) == 1 and len(dec) == 1, names
    return enc[0], dec[0], out["toks"], out["rec"]


@pytest.mark.parametrize("tag", TAGS)
def test_the_routes_the_stride5_layers_ran(tag):
    """Outputs are bit-identical whichever split16 tap-GEMM runs, so nothing above can tell WHICH kernel it judged.  With "prof_detail" on
    the profile records of the two stride-5 launches are read at the shapes of the tests above and at B = 5: in split16 neither runs as the
    exact-fp32 tap_gemm4 (which is all DAC_TINY's N = 80 ever reached); the x5 transposed conv takes the tiny-launch rule's
    tap_gemm8 256 x 128 form up to 64 tiles and the cost model's tap_gemm6 128-column arrangement beyond -- both were run and judged;
    under "fp32_exact" both are tap_gemm4."""
    codec = _codec(tag)
    cfg = _weights(tag)[0]
    seen = set()
    for (B, T), want in ROUTES.items():
        enc, dec, toks, _ = _stride5_records(codec, noise(9500 + T, B, T).cuda())
        print(tag, (B, T), enc, "|", dec)
        assert tuple(toks.shape) == (B, cfg.num_frames(T), cfg.n_codebooks)
        assert (enc, dec) == want, (B, T)
        assert "tap_gemm4" not in enc and "tap_gemm4" not in dec
        assert dec.startswith(TINY8_128) == _tiny_launch(dec) and enc.startswith(TINY8_256) == _tiny_launch(enc)
        seen.add(_tiny_launch(dec))
    assert seen == {True, False}            # the x5 transposed conv: tiny-launch route and cost-model route
    exact = _codec(tag, precision="fp32_exact")
    enc, dec, _, _ = _stride5_records(exact, noise(9500 + 2049, 2, 2049).cuda())
    assert enc == "tap_gemm4_kernel<2, 2, 4, 4> B2 M51 N512 K2560 J2 s5" and dec == "tap_gemm4_kernel<2, 2, 4, 4> B2 M49 N1920 K1536 J2 s1", (enc, dec)


# ------------------------------------------------------------------------------------------------ e. batch independence across routes
# 16 clips x 1 s: (x5 conv alone, in the batch), (x5 transposed conv alone, in the batch).  At 24 kHz one second is 75 frames: the
# transposed conv's 601 rows x 15 column tiles are past the tiny-launch rule even alone, so only the x5 conv changes kernel there.
BATCH_ROUTES = {
    "dac16": ((f"{TINY8_256} B1 M400 N512 K2560 J2 s5", "tap_gemm6_kernel<1, 8, 4, 1, 2> B16 M400 N512 K2560 J2 s5"),
              (f"{TINY8_128} B1 M401 N1920 K1536 J2 s1", "tap_gemm6_kernel<1, 4, 4, 1, 2> B16 M401 N1920 K1536 J2 s1")),
    "dac24": ((f"{TINY8_256} B1 M600 N512 K2560 J2 s5", "tap_gemm6_kernel<1, 8, 4, 1, 2> B16 M600 N512 K2560 J2 s5"),
              ("tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M601 N1920 K1536 J2 s1", "tap_gemm6_kernel<1, 4, 4, 1, 2> B16 M601 N1920 K1536 J2 s1")),
}


@pytest.mark.parametrize("tag", TAGS)
def test_batch_independence_across_routes(tag):
    """A clip alone takes the tiny-launch routes, in a batch of 16 the cost model's: other tiles, the same arithmetic in the same
    order.  Clip 3 alone equals its rows in the batch bit for bit -- tokens, encoder features, waveform -- and a repeated call repeats
    the bits."""
    cfg = _weights(tag)[0]
    codec = _codec(tag)
    sig = noise(9600 + cfg.sampling_rate // 1000, 16, cfg.sampling_rate).cuda()
    enc_b, dec_b, toks, rec = _stride5_records(codec, sig)
    enc_1, dec_1, toks1, rec1 = _stride5_records(codec, sig[3:4], toks[3:4])
    print(tag, enc_1, "|", enc_b, "|", dec_1, "|", dec_b)
    assert ((enc_1, enc_b), (dec_1, dec_b)) == BATCH_ROUTES[tag]
    assert enc_1.split(" B")[0] != enc_b.split(" B")[0]
    assert tuple(toks.shape) == (16, cfg.num_frames(cfg.sampling_rate), cfg.n_codebooks)
    assert torch.equal(toks1, toks[3:4])
    assert torch.equal(rec1, rec[3:4])
    feats = codec.sig_to_feats(sig)
    assert torch.equal(codec.sig_to_feats(sig[3:4]), feats[3:4])
    assert torch.equal(codec.sig_to_toks(sig), toks) and torch.equal(codec.toks_to_sig(toks), rec) and torch.equal(codec.sig_to_feats(sig), feats)


# ------------------------------------------------------------------------------------------------ f. the wrapper as the reference calls it
def test_wrapper_picks_the_model_from_orig_sample_rate():
    from audiocodecs_amd import DAC
    from audiocodecs_amd.config import DAC_16KHZ, DAC_24KHZ, DAC_44KHZ
    from audiocodecs_amd.resample import resample

    cfg16, sd16, _, _ = _weights("dac16")
    assert DAC(16000, state_dict=sd16).config is DAC_16KHZ                       # the default orig_sample_rate
    for sr, orig, cfg in ((16000, 16000, DAC_16KHZ), (24000, 24000, DAC_24KHZ), (44100, 44100, DAC_44KHZ), (16000, 24000, DAC_24KHZ)):
        assert DAC(sr, orig, state_dict=sd16).config is cfg                      # (no handle yet: the weights are not looked at)
    with pytest.raises(ValueError, match="no DAC model for 48000 Hz"):
        DAC(48000, 48000, state_dict=sd16)
    # the default model behind a 24 kHz caller: resample in, native encode and decode, resample out
    outer = DAC(24000, state_dict=sd16, num_codebooks=12).eval()
    native = _codec("dac16")
    assert outer.config is DAC_16KHZ and outer.orig_sample_rate == 16000 and native.sample_rate == native.orig_sample_rate == 16000
    T = 24000 + 7
    sig = noise(9700, 2, T).cuda()
    rec = outer(sig)
    want = resample(native.toks_to_sig(native.sig_to_toks(resample(sig, 24000, 16000))), 16000, 24000)
    assert torch.equal(rec, want)
    L = math.ceil(T * 2 / 3)                                                     # ceil at every rate change (resample.py)
    N = cfg16.num_frames(L)
    assert rec.shape == (2, math.ceil(cfg16.num_samples(N) * 3 / 2)) and bool(torch.isfinite(rec).all())
    assert torch.equal(outer.sig_to_toks(sig), native.sig_to_toks(resample(sig, 24000, 16000))) and outer.sig_to_toks(sig).shape == (2, N, 12)


@pytest.mark.parametrize("tag", TAGS)
def test_codebook_clamp_and_embs_shapes(tag):
    from audiocodecs_amd import DAC

    cfg, sd, _, _ = _weights(tag)
    K = cfg.n_codebooks
    assert K == {"dac16": 12, "dac24": 32}[tag]
    many = DAC(cfg.sampling_rate, cfg.sampling_rate, num_codebooks=50, state_dict=sd).eval()       # upstream's loop just runs out of quantisers
    sig = noise(9800, 2, 2049).cuda()
    toks = many.sig_to_toks(sig)
    assert many.config is cfg and toks.shape == (2, 6, K)
    assert torch.equal(toks, _codec(tag).sig_to_toks(sig))
    assert many.embs().shape == (K, 1024, cfg.hidden_size) == (K, 1024, 1024)
    assert _codec(tag, latent=True).embs().shape == (K, 1024, 8)
    assert _codec(tag, K=8).embs().shape == (8, 1024, 1024) and _codec(tag, K=8, latent=True).embs().shape == (8, 1024, 8)
    assert torch.equal(_codec(tag, K=8).embs(), many.embs()[:8])


# ------------------------------------------------------------------------------------------------ g. a bad token id in the last codebook
@pytest.mark.parametrize("tag", TAGS)
def test_out_of_range_token_id_in_the_last_codebook(tag):
    """F.embedding raises on an id outside the codebook.  No entry point synchronises, so (as for every codec here:
    tests/test_gpu_parity.py::test_out_of_range_token_ids_are_reported) the gather sets the frame to NaN, the NEXT call on the handle
    fails once with AC_EINVAL, and the handle works again afterwards.  Here the id sits in the LAST of 12 / 32 codebooks of one clip:
    that clip's decode is NaN around the frame, the other clips' are untouched to the bit."""
    from audiocodecs_amd._native import NativeError

    cfg = _weights(tag)[0]
    K, hop = cfg.n_codebooks, cfg.hop_length
    codec = _codec(tag)
    toks = torch.randint(0, 1024, (3, 6, K), generator=torch.Generator().manual_seed(9900 + K)).cuda()
    good = codec.toks_to_sig(toks)
    bad = toks.clone()
    bad[1, 2, K - 1] = 1024
    rec = codec.toks_to_sig(bad)
    torch.cuda.synchronize()
    assert rec.shape == good.shape == (3, cfg.num_samples(6)) and bool(torch.isfinite(good).all())
    assert bool(torch.isnan(rec[1, 2 * hop : 3 * hop - 8]).all())                 # the frame's own samples
    assert torch.equal(rec[0], good[0]) and torch.equal(rec[2], good[2])
    with pytest.raises(NativeError, match="token ids outside"):
        codec.toks_to_sig(toks)
    assert torch.equal(codec.toks_to_sig(toks), good)
