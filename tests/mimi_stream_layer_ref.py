"""An fp64 (or fp32) statement of ONE sub-layer of the streamed Mimi transformer (plain torch, no GPU).

The streamed transformer (csrc/mimi_stream.hip) runs a layer as  LN1 + qkv + RoPE  ->  attention over [ring || this push's keys]
->  o-proj ... fc2  and emits the three results through the capture hook (include/audiocodecs_amd.h, ac_debug_capture).  Each
function here is the same step on the CPU, in the dtype of its weights / inputs, stated on ABSOLUTE positions: no ring, no slot
map, no launch order.  `chain` strings them over a push schedule; tests/test_mimi_stream_layers_cpu.py proves that chain equal to
`mimi_oracle.transformer_layer` run one-shot, and tests/test_mimi_stream_layers_gpu.py holds every GPU tap to one function, fed
with the GPU's own earlier taps."""
import math

import torch
import torch.nn.functional as F

from oracle import mimi_oracle as O


def _sizes(cfg):
    nh, hd = cfg.num_attention_heads, cfg.head_dim
    return nh, hd, nh * hd


def qkv_rot(cfg, W, l, part, x_in, pos0):
    """x_in [B,T,H] whose first row sits at absolute position pos0 -> [B,T,3A]: rotated q | rotated k | v.
    LN1, the three projections, RoPE with the angle as `mimi_oracle.rope_tables` defines it (an fp32 product of inv_freq and the
    position, as the model does); everything else in the dtype of W."""
    p = f"{part}.layers.{l}"
    B, T, H = x_in.shape
    nh, hd, A = _sizes(cfg)
    dt = W[p + ".self_attn.q_proj.weight"].dtype
    x = x_in.to(dt)
    h = F.layer_norm(x, (H,), W[p + ".input_layernorm.weight"], W[p + ".input_layernorm.bias"], cfg.norm_eps)
    cos, sin = O.rope_tables(cfg, T, dt, int(pos0))          # [T, hd]
    cos, sin = cos[:, None, :], sin[:, None, :]
    out = []
    for name in ("q", "k", "v"):
        y = F.linear(h, W[p + f".self_attn.{name}_proj.weight"]).view(B, T, nh, hd)
        if name != "v":
            y = y * cos + O._rotate_half(y) * sin
        out.append(y.reshape(B, T, A))
    return torch.cat(out, -1)


def attend(cfg, q_rot, k_hist, v_hist, k_new, v_new, pos0, window=None):
    """q_rot, k_new, v_new [B,T,A]: this push's rows, the first at absolute position pos0.  k_hist, v_hist [B,pos0,A]: the rows of
    the stream's earlier pushes since its last reset, indexed by absolute position.  The query at position p sees the keys j <= p
    with p - j < sliding_window, and no key below position 0.  Softmax and PV in the dtype of the inputs.  -> [B,T,A].
    (`window`: another window, for the sensitivity checks.)"""
    B, T, A = q_rot.shape
    nh, hd, _ = _sizes(cfg)
    win = cfg.sliding_window if window is None else window
    pos0 = int(pos0)
    assert k_hist.shape[1] == pos0 and v_hist.shape[1] == pos0, (tuple(k_hist.shape), pos0)
    lo = max(0, pos0 - (win - 1))                           # the oldest position any query of this push can see
    k = torch.cat([k_hist[:, lo:], k_new], 1)
    v = torch.cat([v_hist[:, lo:], v_new], 1)
    J = k.shape[1]
    q = q_rot.view(B, T, nh, hd).transpose(1, 2)
    k = k.view(B, J, nh, hd).transpose(1, 2)
    v = v.view(B, J, nh, hd).transpose(1, 2)
    p = pos0 + torch.arange(T)[:, None]
    j = lo + torch.arange(J)[None, :]
    visible = (j <= p) & (p - j < win)
    bias = torch.zeros(T, J, dtype=q.dtype).masked_fill(~visible, float("-inf"))
    a = torch.matmul(q, k.transpose(2, 3)) * (1.0 / math.sqrt(hd)) + bias
    a = F.softmax(a, dim=-1)
    return torch.matmul(a, v).transpose(1, 2).reshape(B, T, A)


def layer_out(cfg, W, l, part, x_in, att):
    """x_in [B,T,H] (the layer's input), att [B,T,A] -> the layer's output: o-proj, layer scale, residual, LN2, fc1, exact-erf
    GELU, fc2, layer scale, residual."""
    p = f"{part}.layers.{l}"
    H = x_in.shape[-1]
    dt = W[p + ".self_attn.o_proj.weight"].dtype
    x = x_in.to(dt)
    x = x + W[p + ".self_attn_layer_scale.scale"] * F.linear(att.to(dt), W[p + ".self_attn.o_proj.weight"])
    h = F.layer_norm(x, (H,), W[p + ".post_attention_layernorm.weight"], W[p + ".post_attention_layernorm.bias"], cfg.norm_eps)
    h = F.linear(F.gelu(F.linear(h, W[p + ".mlp.fc1.weight"])), W[p + ".mlp.fc2.weight"])
    return x + W[p + ".mlp_layer_scale.scale"] * h


def upsample(cfg, W, qf_prev_row, qf):
    """qf [B,F,H] (this push's dequantised rows), qf_prev_row [B,H] (the previous push's last row; None = zeros, a fresh stream)
    -> [B,F*stride,H]: the depthwise transposed conv as `mimi_oracle.upsample` states it, run on [previous row | qf] with the
    previous row's own outputs dropped."""
    dt = W["upsample.conv.weight"].dtype
    qf = qf.to(dt)
    prev = torch.zeros_like(qf[:, 0]) if qf_prev_row is None else qf_prev_row.to(dt)
    z = torch.cat([prev[:, None], qf], 1).transpose(1, 2)           # [B,H,F+1]
    y = O.upsample(cfg, W)[1](z)                                     # [B,H,(F+1)*stride]
    return y[..., cfg.resample_stride:].transpose(1, 2)


def chain(cfg, W, part, x_pushes, pos0=0, k_hist=None, v_hist=None):
    """One stream group (B streams at one common position) through every layer of `part`, push by push.  x_pushes: a list of
    [B,T_i,H], the transformer's input of each push.  Returns (taps, k_hist, v_hist): taps[i][l] = {"in", "qkv", "att", "out",
    "pos0"} of push i, layer l; k_hist / v_hist: per layer [B,position,A], to continue from."""
    nl = cfg.num_hidden_layers
    _, _, A = _sizes(cfg)
    B = x_pushes[0].shape[0]
    dt = W[f"{part}.layers.0.self_attn.q_proj.weight"].dtype
    if k_hist is None:
        assert pos0 == 0
        k_hist = [torch.zeros(B, 0, A, dtype=dt) for _ in range(nl)]
        v_hist = [torch.zeros(B, 0, A, dtype=dt) for _ in range(nl)]
    taps = []
    for x in x_pushes:
        x = x.to(dt)
        per_layer = []
        for l in range(nl):
            qkv = qkv_rot(cfg, W, l, part, x, pos0)
            q, k, v = qkv[..., :A], qkv[..., A:2 * A], qkv[..., 2 * A:]
            att = attend(cfg, q, k_hist[l], v_hist[l], k, v, pos0)
            out = layer_out(cfg, W, l, part, x, att)
            per_layer.append({"in": x, "qkv": qkv, "att": att, "out": out, "pos0": pos0})
            k_hist[l] = torch.cat([k_hist[l], k], 1)
            v_hist[l] = torch.cat([v_hist[l], v], 1)
            x = out
        taps.append(per_layer)
        pos0 += x.shape[1]
    return taps, k_hist, v_hist
