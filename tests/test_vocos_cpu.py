"""CPU side of the Vocos decoder for EnCodec tokens (`Encodec(use_vocos=True)`): the synthetic checkpoint, the ABI struct and
entry point, the constructor's mode rules, the bandwidth check at the call, and the fp32 restatement against fp64."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vocos_ref as R
from conftest import ROOT


def _cfgs():
    from audiocodecs_amd.config import VOCOS_ENCODEC_24KHZ, VOCOS_TINY

    return {"full": VOCOS_ENCODEC_24KHZ, "tiny": VOCOS_TINY}


def test_published_shape_constants():
    c = _cfgs()["full"]
    assert (c.input_channels, c.backbone_dim, c.intermediate_dim, c.num_layers, c.adanorm_num_embeddings) == (128, 384, 1152, 8, 4)
    assert (c.n_fft, c.hop_length, c.max_codebooks, c.codebook_size) == (1280, 320, 16, 1024)
    t = _cfgs()["tiny"]
    assert (t.input_channels, t.backbone_dim, t.intermediate_dim, t.num_layers, t.n_fft, t.hop_length) == (16, 256, 512, 2, 1280, 320)


@pytest.mark.parametrize("name", ["tiny", "full"])
def test_generator_keys_shapes_and_determinism(name):
    from audiocodecs_amd import checkpoint

    cfg = _cfgs()[name]
    sd = checkpoint.synthetic_vocos_state_dict(cfg, seed=3)
    C_, I = cfg.backbone_dim, cfg.intermediate_dim
    want = {
        "feature_extractor.codebook_weights": (cfg.max_codebooks * cfg.codebook_size, cfg.input_channels),
        "backbone.embed.weight": (C_, cfg.input_channels, 7), "backbone.embed.bias": (C_,),
        "backbone.norm.scale.weight": (4, C_), "backbone.norm.shift.weight": (4, C_),
        "backbone.final_layer_norm.weight": (C_,), "backbone.final_layer_norm.bias": (C_,),
        "head.out.weight": (cfg.n_fft + 2, C_), "head.out.bias": (cfg.n_fft + 2,), "head.istft.window": (cfg.n_fft,),
    }
    for l in range(cfg.num_layers):
        p = f"backbone.convnext.{l}"
        want.update({f"{p}.dwconv.weight": (C_, 1, 7), f"{p}.dwconv.bias": (C_,), f"{p}.norm.scale.weight": (4, C_),
                     f"{p}.norm.shift.weight": (4, C_), f"{p}.pwconv1.weight": (I, C_), f"{p}.pwconv1.bias": (I,),
                     f"{p}.pwconv2.weight": (C_, I), f"{p}.pwconv2.bias": (C_,), f"{p}.gamma": (C_,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert not any("pos_net" in k for k in sd)
    again = checkpoint.synthetic_vocos_state_dict(cfg, seed=3)
    other = checkpoint.synthetic_vocos_state_dict(cfg, seed=4)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd["backbone.embed.weight"], other["backbone.embed.weight"])
    # the AdaLayerNorm rows differ (a wrong bandwidth row must show) and the tables shrink per stage
    sc = sd["backbone.norm.scale.weight"]
    assert all(not torch.equal(sc[i], sc[j]) for i in range(4) for j in range(i))
    std = sd["feature_extractor.codebook_weights"].view(cfg.max_codebooks, -1).std(dim=1)
    assert bool((std[1:] < std[:-1]).all())


def test_backbone_draws_are_the_wavtokenizer_generators():
    """Backbone and head sit exactly on synthetic_wavtok_state_dict's scales: the same draws under the same names."""
    from audiocodecs_amd import checkpoint
    from audiocodecs_amd.config import WAVTOK_TINY

    v = checkpoint.synthetic_vocos_state_dict(_cfgs()["tiny"], seed=1)
    w = checkpoint.synthetic_wavtok_state_dict(WAVTOK_TINY, seed=1)
    for k in ("backbone.norm.scale.weight", "backbone.convnext.1.pwconv2.weight", "backbone.convnext.0.gamma", "backbone.final_layer_norm.bias"):
        assert torch.equal(v[k], w[k]), k


def test_abi_struct_and_create():
    from audiocodecs_amd import _native

    header = open(os.path.join(ROOT, "include", "audiocodecs_amd.h")).read()
    body = re.search(r"typedef struct ac_vocos_config \{(.*?)\} ac_vocos_config;", header, flags=re.S).group(1)
    fields = re.findall(r"int32_t\s+([a-z_]+);", body)
    assert fields == [f for f, _ in _native.AcVocosConfig._fields_]
    assert C.sizeof(_native.AcVocosConfig) == 4 * len(fields) == 48
    L = _native.lib()
    h = C.c_void_p()
    assert L.ac_vocos_create(C.byref(_native.AcVocosConfig()), C.byref(h)) == -1     # struct_size == 0
    assert L.ac_vocos_create(None, C.byref(h)) == -1
    assert not h.value


def test_encode_mode_needs_no_vocos_weights(checkpoints, monkeypatch):
    from audiocodecs_amd import Encodec

    def no_fetch(tag):
        raise AssertionError("mode='encode' must not fetch Vocos weights")

    monkeypatch.setattr(Encodec, "_fetch_pretrained_vocos", staticmethod(no_fetch))
    cfg, sd = checkpoints("tiny", 0)
    enc = Encodec(24000, mode="encode", use_vocos=True, state_dict=sd, config=cfg)
    assert enc.use_vocos and enc._vocos_sd is None
    assert not any(k.startswith("decoder.") for k in enc._folded)


def test_decoding_modes_drop_the_seanet_decoder(checkpoints):
    from audiocodecs_amd import Encodec, checkpoint

    cfg, sd = checkpoints("tiny", 0)
    vcfg = _cfgs()["tiny"]
    vsd = checkpoint.synthetic_vocos_state_dict(vcfg, seed=0)
    vsd["feature_extractor.encodec.decoder.layers.0.conv.bias"] = torch.zeros(3)      # upstream re-attaches these: ignored
    for mode, enc_kept in (("decode", False), ("reconstruct", True)):
        c = Encodec(24000, mode=mode, use_vocos=True, state_dict=sd, config=cfg, vocos_state_dict=vsd, vocos_config=vcfg)
        assert not any(k.startswith("decoder.") for k in c._folded)
        assert any(k.startswith("encoder.") for k in c._folded) == enc_kept
        assert any(k.startswith("quantizer.") for k in c._folded)
        assert all(k.startswith(("feature_extractor.codebook_weights", "backbone.", "head.")) for k in c._vocos_sd)
    plain = Encodec(24000, mode="decode", state_dict=sd, config=cfg)
    assert plain._vocos_sd is None and any(k.startswith("decoder.") for k in plain._folded)


def test_bandwidth_outside_the_four_raises_at_the_call(checkpoints):
    from audiocodecs_amd import Encodec, checkpoint

    cfg, sd = checkpoints("tiny", 0)
    vcfg = _cfgs()["tiny"]
    c = Encodec(24000, num_codebooks=3, use_vocos=True, state_dict=sd, config=cfg,
                vocos_state_dict=checkpoint.synthetic_vocos_state_dict(vcfg, seed=0), vocos_config=vcfg)
    with pytest.raises(ValueError):
        c.toks_to_sig(torch.zeros(1, 4, 3, dtype=torch.int64))          # a CPU tensor: the bandwidth check comes first
    for k, want in ((2, 0), (4, 1), (8, 2), (16, 3)):
        ok = Encodec(24000, num_codebooks=k, use_vocos=True, state_dict=sd, config=cfg,
                     vocos_state_dict=checkpoint.synthetic_vocos_state_dict(vcfg, seed=0), vocos_config=vcfg)
        assert ok._vocos_bandwidth_id() == want


@pytest.mark.parametrize("name", ["tiny", "full"])
@pytest.mark.parametrize("B,N", [(2, 5), (1, 257)])
def test_fp32_restatement_tracks_fp64(name, B, N):
    """The fp32 evaluation of the restatement (torch's own order) stays within 1e-6 RMS of the fp64 one: the GPU bounds of
    tests/test_vocos_gpu.py (2e-5) are far above what fp32 itself costs on this network."""
    from audiocodecs_amd import checkpoint

    cfg = _cfgs()[name]
    sd = checkpoint.synthetic_vocos_state_dict(cfg, seed=0)
    toks = R.tokens(100 + N, B, N, 8)
    with torch.no_grad():
        t32 = {}
        y32 = R.toks_to_sig(cfg, R.cast(sd), toks, 2, t32)
        y64 = R.toks_to_sig(cfg, R.cast(sd, torch.float64), toks, 2)
    assert y32.shape == (B, N * cfg.hop_length) and y32.dtype == torch.float32
    err = float((y32.double() - y64).square().mean().sqrt())
    assert err < 1e-6, err
    assert float(y64.square().mean().sqrt()) > 1e-3                     # a signal, not silence
    mag = torch.hypot(t32["spec_re"], t32["spec_im"]).max()
    assert float(mag) < 100.0                                           # the clamp at 100 is not what is being compared
