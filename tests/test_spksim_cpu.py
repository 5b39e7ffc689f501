"""CPU tests of the WavLM x-vector speaker encoder's host side (audiocodecs_amd.spksim): the fp64 statement of
tests/spksim_ref.py against transformers' own ``WavLMForXVector`` holding the synthetic weights, the bucket table against the backend's
``_relative_positions_bucket``, the synthetic checkpoint's key layout, the weight-norm fold, the frame and pooled-row rules, and every
refusal that needs no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import spksim_ref as R
from audiocodecs_amd import _native, checkpoint, spksim
from audiocodecs_amd.spksim import WAVLM_BASE_SV, WAVLM_SV_TINY, WavLMSVConfig


def _hf_model(cfg, sd):
    transformers = pytest.importorskip("transformers")
    model = transformers.WavLMForXVector(transformers.WavLMConfig(**cfg.hf_kwargs())).double().eval()
    model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
    return model


def _rel(got, want):
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
def test_statement_equals_transformers_in_fp64(masked):
    """Embeddings and every hidden state to 1e-10 relative, with and without an attention mask."""
    cfg, sd = WAVLM_SV_TINY, R.tiny_state_dict()
    model = _hf_model(cfg, sd)
    L = 12000
    sig = R.clips(3, L).double()
    valid = [L, 9000, 6000] if masked else None
    mask = None
    if masked:
        mask = (torch.arange(L)[None, :] < torch.tensor(valid)[:, None]).long()
    with torch.no_grad():
        out = model(input_values=sig, attention_mask=mask, output_hidden_states=True)
    mine = R.forward(cfg, sd, sig, valid, torch.float64)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1
    for i, hs in enumerate(out.hidden_states):
        assert _rel(mine["hidden"][i], hs) < 1e-10, i
    assert _rel(mine["emb"], out.embeddings) < 1e-10
    assert float(out.embeddings.abs().max()) > 1e-2       # (the synthetic weights keep activations O(1): the comparison means something)


def test_bucket_table_equals_the_backend():
    """Integer equality for every offset at T = 200, for both bucket layouts."""
    transformers = pytest.importorskip("transformers")
    from transformers.models.wavlm.modeling_wavlm import WavLMAttention

    for cfg in (WAVLM_SV_TINY, WAVLM_BASE_SV):
        att = WavLMAttention(cfg.hidden_size, cfg.num_attention_heads, num_buckets=cfg.num_buckets, max_distance=cfg.max_bucket_distance)
        T = 200
        rel = torch.arange(T)[None, :] - torch.arange(T)[:, None]
        want = att._relative_positions_bucket(rel)
        tab = spksim.bucket_table(cfg)
        Rr = 2 * cfg.max_bucket_distance
        assert tab.dtype == torch.int64 and tab.shape == (2 * Rr + 1,)
        assert torch.equal(tab[rel.clamp(-Rr, Rr) + Rr], want)
        # beyond max_distance the buckets are constant: the clamp at the table's ends changes nothing
        far = torch.tensor([[-5 * Rr, -Rr - 1, -Rr, Rr, Rr + 1, 5 * Rr]])
        assert torch.equal(att._relative_positions_bucket(far), tab[far.clamp(-Rr, Rr) + Rr])
        assert int(tab.min()) >= 0 and int(tab.max()) < cfg.num_buckets


def test_synthetic_keys_equal_the_models():
    transformers = pytest.importorskip("transformers")
    for cfg in (WAVLM_SV_TINY,):
        sd = checkpoint.synthetic_wavlm_sv_state_dict(cfg, 0)
        model = transformers.WavLMForXVector(transformers.WavLMConfig(**cfg.hf_kwargs()))
        want = model.state_dict()
        assert set(sd) == set(want)
        for k, v in want.items():
            assert tuple(sd[k].shape) == tuple(v.shape), k
    assert WavLMSVConfig.from_hf(transformers.WavLMConfig(**WAVLM_SV_TINY.hf_kwargs())) == WAVLM_SV_TINY


def test_weight_norm_fold():
    """dim = 2: one norm per tap over (out, in); the synthetic original0 is that norm, so the folded weight is original1."""
    sd = R.tiny_state_dict()
    pc = "wavlm.encoder.pos_conv_embed.conv.parametrizations.weight."
    g, v = sd[pc + "original0"].double(), sd[pc + "original1"].double()
    assert g.shape == (1, 1, WAVLM_SV_TINY.num_conv_pos_embeddings)
    w = spksim.fold_pos_conv_weight_norm(g, v)
    assert torch.allclose(w, torch._weight_norm(v, g, 2), rtol=1e-14, atol=0)
    assert torch.allclose(w, v, rtol=1e-6, atol=0)
    w2 = spksim.fold_pos_conv_weight_norm(2.0 * g, v)
    assert torch.allclose(w2, 2.0 * v, rtol=1e-6, atol=0)


def test_num_frames_and_pooled_rows():
    transformers = pytest.importorskip("transformers")
    model = transformers.WavLMForXVector(transformers.WavLMConfig(**WAVLM_SV_TINY.hf_kwargs()))
    lengths = [399, 400, 401, 719, 720, 721, 4879, 4880, 4881, 5199, 5200, 5201, 41680, 160000]
    for L in lengths:
        want = int(model._get_feat_extract_output_lengths(L)) if L >= 400 else 0
        assert spksim.num_frames(L) == want == R.frames(L), L
    L = 41680
    T = spksim.num_frames(L)
    assert T == 130
    assert spksim.num_pooled_rows(L) == T - 14
    for valid in [L, L - 1, 32000, 20560, 20559, 20880, 4880, 2960, 2959, 2640, 400, 399]:
        lf = int(model._get_feat_extract_output_lengths(valid)) if valid >= 400 else 0
        want = min(int(model._get_tdnn_output_lengths(lf)), T - 14)
        assert spksim.num_pooled_rows(L, valid) == want == R.pooled_rows(L, valid), valid
    assert spksim.num_pooled_rows(4880) == 1 and spksim.num_pooled_rows(4879) == 0 and spksim.num_pooled_rows(5200) == 2


def test_create_refuses_without_gpu():
    L = _native.lib()
    h = C.c_void_p()
    assert L.ac_spk_create(C.byref(_native.AcSpkConfig()), C.byref(h)) == -1       # struct_size == 0
    assert L.ac_spk_create(None, C.byref(h)) == -1

    def rc(cfg):
        c = spksim._struct(cfg)
        c.struct_size = C.sizeof(c)
        c.device = 1 << 20           # (a valid config stops at the device: never created here)
        return L.ac_spk_create(C.byref(c), C.byref(h))

    import dataclasses

    ok = rc(WAVLM_SV_TINY)
    assert ok < -1, ok           # not AC_EINVAL (-1): the config itself passes, the device does not exist
    assert rc(WAVLM_BASE_SV) == ok
    for bad in (dict(do_stable_layer_norm=True), dict(feat_extract_norm="layer"), dict(conv_bias=True), dict(use_weighted_layer_sum=False),
                dict(add_adapter=True), dict(num_attention_heads=4), dict(hidden_size=96), dict(conv_kernel=(10, 3, 3, 3, 3, 3, 2)),
                dict(conv_stride=(5, 2, 2, 2, 2, 2, 1)), dict(num_conv_pos_embeddings=15), dict(tdnn_dilation=(1, 2, 2, 1, 1)),
                dict(conv_dim=48)):
        assert rc(dataclasses.replace(WAVLM_SV_TINY, **bad)) == -1, bad
    assert L.ac_spk_num_frames(399) == 0 and L.ac_spk_num_frames(400) == 1
    assert L.ac_spk_workspace_bytes(None, 1, 16000) == 0
    assert L.ac_spk_cosine(None, None, 1, 4, None, None) == -1


def test_python_refusals():
    sd = R.tiny_state_dict()
    enc = spksim.SpeakerEncoder(state_dict=sd, arch=WAVLM_SV_TINY)
    sig = torch.zeros(2, 8000)
    with pytest.raises(ValueError):
        enc.forward(sig, 0)
    with pytest.raises(ValueError):
        enc.forward(sig, 16000.0)
    with pytest.raises(ValueError):
        enc.forward(sig[0], 16000)
    with pytest.raises(ValueError):
        enc.forward(sig, 16000, lens=torch.ones(3))
    with pytest.raises(ValueError):
        enc.forward(sig, 16000, lens=torch.ones(2, dtype=torch.int64))
    with pytest.raises(_native.NativeError):
        enc.forward(sig, 16000)                               # a CPU tensor: there is no CPU fallback
    with pytest.raises(ValueError):
        enc.embed_16k(torch.zeros(2, 4879))
    with pytest.raises(ValueError):
        enc.embed_16k(torch.zeros(2, 8000), valid=torch.ones(2))
    with pytest.raises(ValueError):
        spksim.SpeakerEncoder(state_dict=sd, arch="tiny")
    with pytest.raises(ValueError):
        spksim.speaker_similarity(sig, sig[:1], 16000, enc)
    with pytest.raises(ValueError):
        spksim.speaker_similarity(sig, sig, 16000, object())
    with pytest.raises(ValueError):
        spksim.speaker_similarity(sig, sig, 16000, spksim.SpeakerEncoder(state_dict=sd, arch=WAVLM_SV_TINY, pool=False))
    with pytest.raises(ValueError):
        spksim.cosine(torch.zeros(2, 4), torch.zeros(3, 4))
    import audiocodecs_amd

    for name in ("SpeakerEncoder", "speaker_similarity", "SpkSimWavLM", "WavLMSVConfig", "WAVLM_BASE_SV", "WAVLM_SV_TINY"):
        assert name in audiocodecs_amd.__all__ and hasattr(audiocodecs_amd, name)


def test_spksim_bookkeeping_with_a_stub(monkeypatch):
    """`append` and `summarize` as the reference class: ids and scores in order, one score per clip."""
    calls = []

    def fake(hyp, ref, sample_rate, encoder, lens=None):
        calls.append((tuple(hyp.shape), sample_rate, encoder, lens))
        return hyp.mean(dim=1)

    monkeypatch.setattr(spksim, "speaker_similarity", fake)
    m = spksim.SpkSimWavLM("unused", 24000, model="stub")
    a = torch.tensor([[0.5, 0.5], [0.25, 0.25]])
    m.append(["a", "b"], a, a)
    m.append(["c"], a[:1] * 0 + 0.75, a[:1], lens=torch.ones(1))
    assert m.ids == ["a", "b", "c"] and m.scores == [0.5, 0.25, 0.75]
    assert calls[0][1:3] == (24000, "stub") and calls[1][3] is not None
    s = m.summarize()
    assert s == {"average": 0.5, "min_score": 0.25, "min_id": "b", "max_score": 0.75, "max_id": "c"}
    assert m.summarize("average") == 0.5
    with pytest.raises(ValueError):
        m.append(["x"], a, a)
    with pytest.raises(ValueError):
        m.append(["x", "y"], a, a[:1])
    m.clear()
    assert m.ids == [] and m.scores == []


def test_fixture_clips_are_told_apart():
    """The four clips of the main GPU case: their fp64 cosines span at least 0.03 (the fp32 error of a cosine there is 1e-7), so a
    similarity that ignored its input would not pass."""
    s = R.forward(WAVLM_SV_TINY, R.tiny_state_dict(), R.clips(4, R.MAIN_L), None, torch.float64)
    e = s["emb"]
    cos = [float(torch.nn.functional.cosine_similarity(e[i], e[j], dim=0)) for i in range(4) for j in range(i + 1, 4)]
    print("fp64 cosines between the fixture clips:", [round(c, 4) for c in cos])
    assert max(cos) - min(cos) >= 0.03
    assert np.isfinite(cos).all()
