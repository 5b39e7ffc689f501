"""GPU parity of the Vocos decode of EnCodec tokens (`Encodec(use_vocos=True).toks_to_sig`, through ac_vocos_create / ac_decode)
against the fp64 restatement of tests/vocos_ref.py.  PARITY UNPINNED w.r.t. the reference (the `vocos` package is not on disk):
what is asserted is HIP path == restatement -- every module output, the waveform within 1e-4 RMS (the north-star bar) and 2e-5
(what this kernel family is held to in tests/test_wavtok_gpu_parity.py; the tolerances are that file's)."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_record
import vocos_ref as R
from golden_cases import noise
from test_wavtok_gpu_parity import check_taps, rms

pytestmark = pytest.mark.gpu

BW_ID = {2: 0, 4: 1, 8: 2, 16: 3}
_SD, _GOLD = {}, {}


def setup(name):
    """(EnCodec config, its state dict, Vocos config, its state dict, fp64 weights) of the tiny / full pair; built once."""
    if name not in _SD:
        from audiocodecs_amd import checkpoint
        from audiocodecs_amd.config import ENCODEC_24KHZ, TINY, VOCOS_ENCODEC_24KHZ, VOCOS_TINY

        cfg, vcfg = {"tiny": (TINY, VOCOS_TINY), "full": (ENCODEC_24KHZ, VOCOS_ENCODEC_24KHZ)}[name]
        vsd = checkpoint.synthetic_vocos_state_dict(vcfg, seed=0)
        _SD[name] = (cfg, checkpoint.synthetic_state_dict(cfg, seed=0), vcfg, vsd, R.cast(vsd, torch.float64))
    return _SD[name]


def make(name, mode="decode", num_codebooks=8, sample_rate=24000, **kw):
    from audiocodecs_amd import Encodec

    cfg, sd, vcfg, vsd, _ = setup(name)
    return Encodec(sample_rate, mode=mode, num_codebooks=num_codebooks, use_vocos=True, state_dict=sd, config=cfg,
                   vocos_state_dict=vsd, vocos_config=vcfg, **kw).eval()


@pytest.fixture(scope="module")
def codecs():
    cache = {}

    def get(name, **kw):
        key = (name, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = make(name, **kw)
        return cache[key]

    return get


def gold(name, toks, bw_id):
    """fp64 restatement: (waveform [B, N*hop], module taps [B,C,N]) as numpy; computed once per input."""
    key = (name, bw_id, tuple(toks.shape), int(toks.sum()))
    if key not in _GOLD:
        taps = {}
        with torch.no_grad():
            y = R.toks_to_sig(setup(name)[2], setup(name)[4], toks, bw_id, taps)
        _GOLD[key] = (y.numpy(), {k: v.numpy() for k, v in taps.items()})
    return _GOLD[key]


def capture(codec, fn, nfloats=1 << 24):
    nat = next(iter(codec._vocos_natives.values()))
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


def check_case(name, codec, B, N, atol, label, K=8, seed=0):
    vcfg = setup(name)[2]
    toks = R.tokens(7000 + 100 * B + N + seed, B, N, K)
    y64, t64 = gold(name, toks, BW_ID[codec.num_codebooks])
    codec.toks_to_sig(toks[:1, :1].cuda())            # the handle exists before the capture buffer is armed
    rec, flat = capture(codec, lambda: codec.toks_to_sig(toks.cuda()))
    assert rec.shape == (B, N * vcfg.hop_length) and rec.dtype == torch.float32
    err = rms(rec.cpu().numpy() - y64)
    print(f"encodec_vocos/{label}: waveform rms err {err:.3e} (signal rms {rms(y64):.3e})")
    worst = None
    try:
        worst = check_taps(flat, R.tap_names(vcfg), lambda t: t64[t], atol)
    finally:
        parity_record.record("encodec_vocos", label, waveform_rms_err=err, worst_rel_err_per_tap=worst)
    assert err < 1e-4, err          # the north-star bar
    assert err < 2e-5, err


@pytest.mark.parametrize("B,N", [(2, 1), (2, 3), (3, 5), (2, 17)])
def test_tiny_every_module_output_and_waveform(B, N, codecs):
    """Fewer frames than the k7 halo and than the 4 iSTFT taps, a clip boundary inside a 4-row dwconv_ln workgroup, the 16-row seam + 1."""
    check_case("tiny", codecs("tiny"), B, N, 5e-6, f"tiny_B{B}_N{N}")


@pytest.mark.parametrize("B,N", [(2, 1), (3, 75), (1, 255), (1, 257)])
def test_full_config_waveform_and_taps(B, N, codecs):
    """128 / 384 / 1152 / 8 layers / n_fft 1280: N = 384, 1152 and 1344 columns on the 128- and 256-column tiles; 255 / 257 rows straddle the 256-row tile."""
    check_case("full", codecs("full"), B, N, 1e-5, f"full_B{B}_N{N}")


def test_fp32_exact_precision(codecs):
    check_case("full", codecs("full", precision="fp32_exact"), 3, 75, 1e-5, "full_B3_N75_fp32_exact")


def test_adalayernorm_row_follows_num_codebooks(codecs):
    """ids 0..3 for 2 / 4 / 8 / 16 codebooks on ONE token tensor (K comes from the tensor); the generator's rows differ, so do the outputs."""
    toks = R.tokens(31, 2, 9, 2)
    outs = []
    for k in (2, 4, 8, 16):
        rec = codecs("tiny", num_codebooks=k).toks_to_sig(toks.cuda()).cpu().numpy()
        err = rms(rec - gold("tiny", toks, BW_ID[k])[0])
        parity_record.record("encodec_vocos", f"tiny_row_nq{k}", waveform_rms_err=err)
        assert err < 2e-5, (k, err)
        outs.append(rec)
    for i in range(4):
        for j in range(i):
            assert rms(outs[i] - outs[j]) > 1e-3, (i, j)


def test_table_count_comes_from_the_tensor(codecs):
    from audiocodecs_amd._native import NativeError

    codec = codecs("tiny")                              # num_codebooks = 8: AdaLayerNorm row 2
    toks = R.tokens(32, 2, 6, 8)
    rec = codec.toks_to_sig(toks[..., :3].cuda()).cpu().numpy()
    err = rms(rec - gold("tiny", toks[..., :3].contiguous(), 2)[0])
    assert err < 2e-5, err
    assert rms(rec - codec.toks_to_sig(toks.cuda()).cpu().numpy()) > 1e-3
    with pytest.raises((ValueError, NativeError)):
        codec.toks_to_sig(torch.zeros(1, 4, 17, dtype=torch.int64, device="cuda"))
    assert codec.toks_to_sig(toks[:0].cuda()).shape == (0, 6 * 320)        # an empty shard


def test_clips_are_independent(codecs):
    codec = codecs("full")
    toks = R.tokens(33, 5, 21, 8).cuda()
    whole = codec.toks_to_sig(toks)
    parts = torch.cat([codec.toks_to_sig(toks[b : b + 1]) for b in range(5)])
    assert torch.equal(whole, parts)


def test_bad_token_id(codecs):
    """An id outside [0, 1024) behaves as in ac_decode: the frame is NaN, the other clips are untouched, the next call on the
    handle reports it once; strict=True makes the offending call itself raise."""
    from audiocodecs_amd._native import NativeError

    codec = make("tiny")
    toks = R.tokens(34, 3, 12, 8).cuda()
    clean = codec.toks_to_sig(toks)
    bad = toks.clone()
    bad[1, 5, 2] = 1024
    rec = codec.toks_to_sig(bad)
    torch.cuda.synchronize()
    assert torch.equal(rec[0], clean[0]) and torch.equal(rec[2], clean[2])
    assert bool(torch.isnan(rec[1]).any())
    with pytest.raises(NativeError, match="token ids outside"):
        codec.toks_to_sig(toks)
    assert torch.equal(codec.toks_to_sig(toks), clean)
    strict = make("tiny", strict=True)
    assert torch.equal(strict.toks_to_sig(toks), clean)
    with pytest.raises(NativeError, match="token ids outside"):
        strict.toks_to_sig(bad)
    assert torch.equal(strict.toks_to_sig(toks), clean)


def test_modes(codecs):
    from audiocodecs_amd import Encodec
    from audiocodecs_amd._native import NativeError

    cfg, sd, vcfg, vsd, _ = setup("tiny")
    dec = codecs("tiny")
    plain = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    sig = noise(35, 2, 4000).cuda()
    toks = plain.sig_to_toks(sig)
    with pytest.raises(NativeError, match="without encoder weights"):
        dec.sig_to_toks(sig)
    assert torch.equal(dec.embs(), plain.embs()) and torch.equal(dec.toks_to_qfeats(toks), plain.toks_to_qfeats(toks))
    both = codecs("tiny", mode="reconstruct")
    assert torch.equal(both.sig_to_toks(sig), toks)
    assert torch.equal(both(sig), both.toks_to_sig(toks)) and torch.equal(both.toks_to_sig(toks), dec.toks_to_sig(toks))
    assert not torch.equal(both.toks_to_sig(toks), plain.toks_to_sig(toks))            # Vocos, not SEANet
    enc = make("tiny", mode="encode")
    assert torch.equal(enc(sig), toks)
    with pytest.raises(NativeError, match="without decoder weights"):
        enc.toks_to_sig(toks)
    c16 = make("tiny", mode="reconstruct", sample_rate=16000)
    assert c16(noise(36, 1, 3200).cuda()).shape == (1, 3200)


def test_graph_mode_replays_the_vocos_decode(codecs):
    eager = codecs("tiny", mode="reconstruct")
    g = make("tiny", mode="reconstruct", graph=True)
    for seed in (40, 41, 42):
        toks = R.tokens(seed, 2, 25, 8).cuda()
        assert torch.equal(g.toks_to_sig(toks), eager.toks_to_sig(toks))
    assert [k[0] for k in g._graphs] == ["toks_to_sig"]
    sig = noise(43, 2, 4000).cuda()
    assert torch.equal(g.sig_to_toks(sig), eager.sig_to_toks(sig))                     # declines: eager
    assert [k[0] for k in g._graphs] == ["toks_to_sig"]


def test_profile_sees_the_vocos_handle_and_no_pos_net_kernel(codecs):
    codec = codecs("full")
    toks = R.tokens(44, 2, 40, 8).cuda()
    codec.toks_to_sig(toks)
    names = {r[0] for r in codec.profile_kernels(lambda: codec.toks_to_sig(toks))}
    for k in ("rvq_decode_kernel", "dwconv_ln_kernel", "polar_kernel", "istft_env_kernel"):
        assert k in names, names
    assert not any(n.startswith(("attn1_kernel", "gn_stats_kernel", "gn_apply_kernel")) for n in names), names
