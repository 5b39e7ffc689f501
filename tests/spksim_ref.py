"""The forward pass of transformers' ``WavLMForXVector`` (microsoft/wavlm-base-sv family) stated in plain torch, in a chosen dtype, with
every stage returned.  It imports neither transformers nor the library's kernels; tests/test_spksim_cpu.py pins it (in fp64) to the
transformers class holding the same weights, tests/test_spksim_gpu.py compares the library against it and takes its tolerances from the
difference between this statement in fp32 and in fp64.

Stages (what ``ac_spk_stages`` holds): ``feat`` [B, T, C] behind conv 7, ``hidden`` [layers + 1, B, T, H] (the input of every layer, then
the last output), ``tdnn`` [B, T - 14, last], ``pooled`` [B, 2 last], and ``emb`` [B, D].
"""
import numpy as np
import torch
import torch.nn.functional as F

from audiocodecs_amd import prng
from audiocodecs_amd.spksim import bucket_table, fold_pos_conv_weight_norm

STAGES = ("feat", "hidden", "tdnn", "pooled", "emb")


def frames(L):
    return (L - 400) // 320 + 1 if L >= 400 else 0


def length_for_frames(T):
    return 320 * (T - 1) + 400


def pooled_rows(L, valid=None):
    """Rows the statistic pooling takes: all T - 14 without a mask, min(Lf - 8, T - 14) with one (the backend's formula)."""
    T = frames(L)
    if valid is None:
        return T - 14
    return min(frames(valid) - 8, T - 14)


def weights(sd, dtype, device="cpu"):
    w = {k: v.to(device=device, dtype=dtype) for k, v in sd.items() if v.is_floating_point()}
    pc = "wavlm.encoder.pos_conv_embed.conv"
    w[pc + ".weight"] = fold_pos_conv_weight_norm(w[pc + ".parametrizations.weight.original0"], w[pc + ".parametrizations.weight.original1"])
    return w


def _ln(x, w, prefix, eps):
    return F.layer_norm(x, (x.shape[-1],), w[prefix + ".weight"], w[prefix + ".bias"], eps)


def _lin(x, w, prefix):
    return F.linear(x, w[prefix + ".weight"], w[prefix + ".bias"])


@torch.no_grad()
def forward(cfg, sd, sig, valid=None, dtype=torch.float64):
    """sig [B, L] at 16 kHz, valid: list of B sample counts or None -> dict of the stages (in `dtype`) plus "Lf" and "rows" (lists)."""
    dev = sig.device                                    # (the CPU in the tests; tools/spksim_latency.py runs it on the device)
    w = weights(sd, dtype, dev)
    x = sig.to(dtype)[:, None, :]
    B, L = sig.shape
    C, H, heads, eps = cfg.conv_dim, cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    fx = "wavlm.feature_extractor.conv_layers."
    for i, (k, s) in enumerate(zip(cfg.conv_kernel, cfg.conv_stride)):
        x = F.conv1d(x, w[f"{fx}{i}.conv.weight"], stride=s)
        if i == 0:      # GroupNorm with one group per channel: moments over ALL frames, padding included
            x = F.group_norm(x, C, w[fx + "0.layer_norm.weight"], w[fx + "0.layer_norm.bias"], 1e-5)
        x = F.gelu(x)
    feat = x.transpose(1, 2).contiguous()
    T = feat.shape[1]
    assert T == frames(L)
    Lf = [T] * B if valid is None else [min(frames(int(v)), T) for v in valid]
    h = _lin(_ln(feat, w, "wavlm.feature_projection.layer_norm", eps), w, "wavlm.feature_projection.projection")
    keymask = torch.zeros(B, T, dtype=torch.bool, device=dev)
    for b in range(B):
        keymask[b, Lf[b]:] = True
    if valid is not None:
        h = h.masked_fill(keymask[:, :, None], 0.0)
    K = cfg.num_conv_pos_embeddings
    pc = "wavlm.encoder.pos_conv_embed.conv"
    pos = F.conv1d(h.transpose(1, 2), w[pc + ".weight"], w[pc + ".bias"], padding=K // 2, groups=cfg.num_conv_pos_embedding_groups)
    if K % 2 == 0:
        pos = pos[:, :, :-1]
    h = _ln(h + F.gelu(pos).transpose(1, 2), w, "wavlm.encoder.layer_norm", eps)
    # E[bucket(k - q)][head]: layer 0's embedding, shared by all layers
    tab = bucket_table(cfg).to(dev)
    R = 2 * cfg.max_bucket_distance
    delta = (torch.arange(T, device=dev)[None, :] - torch.arange(T, device=dev)[:, None]).clamp(-R, R) + R
    bias = w["wavlm.encoder.layers.0.attention.rel_attn_embed.weight"][tab[delta]].permute(2, 0, 1)      # [heads, q, k]
    hidden = [h]
    for l in range(cfg.num_hidden_layers):
        p = f"wavlm.encoder.layers.{l}"
        a = p + ".attention"
        xh = h.view(B, T, heads, 64).permute(0, 2, 1, 3)                                   # the layer's INPUT, per head
        pr = F.linear(xh, w[a + ".gru_rel_pos_linear.weight"], w[a + ".gru_rel_pos_linear.bias"]).view(B, heads, T, 2, 4).sum(-1)
        ga, gb = torch.sigmoid(pr).chunk(2, dim=-1)
        gate = ga * (gb * w[a + ".gru_rel_pos_const"] - 1.0) + 2.0                          # [B, heads, T, 1]
        q = _lin(h, w, a + ".q_proj").view(B, T, heads, 64).permute(0, 2, 1, 3)
        k = _lin(h, w, a + ".k_proj").view(B, T, heads, 64).permute(0, 2, 1, 3)
        v = _lin(h, w, a + ".v_proj").view(B, T, heads, 64).permute(0, 2, 1, 3)
        score = (q * 0.125) @ k.transpose(-1, -2) + gate * bias[None]
        score = score.masked_fill(keymask[:, None, None, :], float("-inf"))
        att = (torch.softmax(score, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, T, H)
        h = _ln(h + _lin(att, w, a + ".out_proj"), w, p + ".layer_norm", eps)
        ff = _lin(F.gelu(_lin(h, w, p + ".feed_forward.intermediate_dense")), w, p + ".feed_forward.output_dense")
        h = _ln(h + ff, w, p + ".final_layer_norm", eps)
        hidden.append(h)
    hidden = torch.stack(hidden)
    lw = torch.softmax(w["layer_weights"], dim=-1)
    x = (hidden * lw.view(-1, 1, 1, 1)).sum(0)
    x = _lin(x, w, "projector")
    for i, (k, d) in enumerate(zip(cfg.tdnn_kernel, cfg.tdnn_dilation)):
        wt = w[f"tdnn.{i}.kernel.weight"]
        x = F.conv1d(x.transpose(1, 2), wt.view(wt.shape[0], k, -1).transpose(1, 2), w[f"tdnn.{i}.kernel.bias"], dilation=d).transpose(1, 2)
        x = torch.relu(x)
    rows = [T - 14] * B if valid is None else [min(lf - 8, T - 14) for lf in Lf]
    if min(rows) < 1:
        raise ValueError(f"pooled rows {rows}: a clip has none")
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # (std of one row: NaN, as the backend)
        pooled = torch.stack([torch.cat([x[b, :n].mean(0), x[b, :n].std(0)]) for b, n in enumerate(rows)])
    emb = _lin(pooled, w, "feature_extractor")
    return {"feat": feat, "hidden": hidden, "tdnn": x.contiguous(), "pooled": pooled, "emb": emb, "Lf": Lf, "rows": rows}


def stage_errors(cfg, sd, sig, valid=None):
    """(fp64 stages, {stage: largest |fp32 statement - fp64 statement|}): the yardstick of a comparison on these inputs."""
    s64 = forward(cfg, sd, sig, valid, torch.float64)
    s32 = forward(cfg, sd, sig, valid, torch.float32)
    err = {}
    for k in STAGES:
        d = (s32[k].double() - s64[k]).abs()
        d = d[~torch.isnan(s64[k])]
        err[k] = float(d.max()) if d.numel() else 0.0
    return s64, err


def clips(B, L, seed=0):
    """B different clips of L samples at 16 kHz, fp32: noise, two tones, a random walk, then mixtures of them with noise."""
    t = np.arange(L) / 16000.0
    base = [
        prng.normal(seed, "spk.noise", (L,)) * 0.1,
        0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.1 * np.sin(2 * np.pi * 660.0 * t),
        0.2 * np.sin(2 * np.pi * 1000.0 * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t)) + 0.1 * np.sin(2 * np.pi * 3100.0 * t),
        None,
    ]
    walk = np.cumsum(prng.normal(seed, "spk.walk", (L,)))
    walk = walk - np.linspace(walk[0], walk[-1], L)
    base[3] = 0.3 * walk / max(np.abs(walk).max(), 1e-9)
    out = []
    for b in range(B):
        x = base[b % 4]
        if b >= 4:
            x = 0.7 * x + prng.normal(seed, f"spk.mix{b}", (L,)) * 0.05
        out.append(x)
    return torch.from_numpy(np.stack(out).astype(np.float32))


MAIN_L = 41680                                   # T = 130: beyond the tiny model's bucket clamp at 80 and over two key tiles
MAIN_VALID = [MAIN_L, 32000, 20560, MAIN_L]      # Lf = 130, 99, 64 (a tile edge), 130: the full-length masked clips hit min(Lf - 8, T - 14)

_SD = {}


def tiny_state_dict(seed=0):
    from audiocodecs_amd import checkpoint
    from audiocodecs_amd.spksim import WAVLM_SV_TINY

    if seed not in _SD:
        _SD[seed] = checkpoint.synthetic_wavlm_sv_state_dict(WAVLM_SV_TINY, seed)
    return _SD[seed]
