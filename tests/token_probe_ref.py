"""The statement of `TokenProbe` (audiocodecs_amd.probe) in torch, by dtype: the multi-codebook embedding and the
pooling in the reference's arithmetic (downstream/models/multihead.py, pooling.py), `torch.nn.LSTM` on packed sequences, the two heads and
the CTC greedy collapse.  Shared by the CPU test, the GPU test, tools/make_token_probe_golden.py and tools/token_probe_latency.py.

fp64 is the yardstick and the same statement in fp32 supplies each bound, as in llama_ref: K_BOUND times its error for a tensor; an arg-max
has to agree wherever the fp64 top-two gap exceeds GAP_FACTOR times the fp32 statement's logit error, and the frames that rule leaves out
are counted against CAP (llama_score_ref's).

speechbrain's wrappers are restated, not pinned: `RNN.LSTM` called with lengths packs the sequences (a clip of length 0, which
`pack_padded_sequence` refuses, is all zeros here); `StatisticsPooling` is the mean and the unbiased std over the valid frames without
its 1e-5-scale jitter; `ctc_greedy_decode` is groupby, then dropping the blank.
"""
import dataclasses

import numpy as np
import torch

from audiocodecs_amd import prng
from audiocodecs_amd.probe import PROBE_TINY, ProbeConfig, weight_names

K_BOUND, GAP_FACTOR = 8.0, 16.0
CAP = 0.03          # llama_score_ref.CAP (asserted equal in the CPU test)

TINY = PROBE_TINY
RECIPE = ProbeConfig(vocab_size=1024, num_codebooks=2, embedding_dim=128, hidden_size=512, num_layers=2, pooling="linear", head="ctc", num_classes=1001)
CONFIGS = {
    "TINY": TINY,
    "TINY_ATT": dataclasses.replace(TINY, pooling="attentional", padding_idx=True),
    "TINY_UTT": dataclasses.replace(TINY, head="utterance", num_classes=7),
    "TINY_FEATS": dataclasses.replace(TINY, pooling=None, head="utterance", num_classes=7),
    "RECIPE": RECIPE,
    "RECIPE_ATT": dataclasses.replace(RECIPE, pooling="attentional"),
}

# the cases of the GPU test: name -> (configuration, B, N, lengths or None)
MIXED35 = [19, 1, 7, 0, 12, 19, 3, 18, 5, 16, 2, 19, 9, 11, 4, 17, 19, 6, 13, 8, 1, 15, 10, 14, 19, 2, 0, 18, 7, 12, 3, 16, 19, 5, 9]
CASES = {
    "tiny3": ("TINY", 3, 37, [37, 20, 1]),
    "tiny35": ("TINY", 35, 19, MIXED35),
    "att3": ("TINY_ATT", 3, 37, [37, 20, 1]),
    "utt3": ("TINY_UTT", 3, 37, [37, 20, 5]),
    "feats3": ("TINY_FEATS", 3, 37, [37, 20, 5]),
    "recipe": ("RECIPE", 2, 75, [75, 41]),
    "recipe_att": ("RECIPE_ATT", 2, 75, [75, 41]),
}

_WEIGHTS = {}


def weights(cfg, seed=0):
    """A synthetic state dict under torch's names: a unit-variance table, projections of variance 1 / fan_in (gate pre-activations near
    unit spread), small biases, a head whose logits spread near 1."""
    key = (cfg, seed)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    H, E = cfg.hidden_size, cfg.embedding_dim

    def t(name, shape, scale):
        return torch.from_numpy((prng.normal(seed, "probe." + name, shape) * scale).astype(np.float32))

    sd = {}
    if cfg.pooling is not None:
        sd["embedding.weight"] = t("embedding.weight", (cfg.table_rows, E), 1.0)
    if cfg.pooling == "linear" and cfg.num_codebooks > 1:
        sd["pooling.mlp.weight"] = t("pooling.mlp.weight", (1, cfg.num_codebooks), 1.0)
    if cfg.pooling == "attentional":
        sd["pooling.attn_mlp.0.weight"] = t("pooling.attn_mlp.0.weight", (E, E), 1.0 / np.sqrt(E))
        sd["pooling.attn_mlp.0.bias"] = t("pooling.attn_mlp.0.bias", (E,), 0.1)
        sd["pooling.attn_mlp.2.weight"] = t("pooling.attn_mlp.2.weight", (1, E), 2.0 / np.sqrt(E))
    for l in range(cfg.num_layers):
        fan = E if l == 0 else 2 * H
        for sfx in ("", "_reverse"):
            sd[f"encoder.rnn.weight_ih_l{l}{sfx}"] = t(f"weight_ih_l{l}{sfx}", (4 * H, fan), 1.0 / np.sqrt(fan))
            sd[f"encoder.rnn.weight_hh_l{l}{sfx}"] = t(f"weight_hh_l{l}{sfx}", (4 * H, H), 1.0 / np.sqrt(H))
            sd[f"encoder.rnn.bias_ih_l{l}{sfx}"] = t(f"bias_ih_l{l}{sfx}", (4 * H,), 0.1)
            sd[f"encoder.rnn.bias_hh_l{l}{sfx}"] = t(f"bias_hh_l{l}{sfx}", (4 * H,), 0.1)
    sd["head.weight"] = t("head.weight", (cfg.num_classes, cfg.head_in), 6.0 / np.sqrt(cfg.head_in))
    sd["head.bias"] = t("head.bias", (cfg.num_classes,), 0.1)
    assert sorted(sd) == sorted(weight_names(cfg))
    _WEIGHTS[key] = sd
    return sd


def inputs(cfg, B, N, seed=1):
    """toks [B, N, K] int64 (with `padding_idx`, a few ids equal to vocab_size), or features [B, N, E] fp32 without pooling."""
    if cfg.pooling is None:
        return torch.from_numpy(prng.normal(seed, "probe.feats", (B, N, cfg.embedding_dim)).astype(np.float32))
    toks = torch.from_numpy(prng.randint(seed, "probe.toks", [B, N, cfg.num_codebooks], cfg.vocab_size))
    if cfg.padding_idx:
        pad = torch.from_numpy(prng.randint(seed, "probe.toks.pad", [B, N, cfg.num_codebooks], 8)) == 0
        toks = torch.where(pad, torch.full_like(toks, cfg.vocab_size), toks)
    return toks


def argmax_lowest(logits):
    """The arg-max with the lowest index on a tie."""
    C = logits.shape[-1]
    idx = torch.arange(C, device=logits.device).expand_as(logits)
    return torch.where(logits == logits.amax(dim=-1, keepdim=True), idx, torch.full_like(idx, C)).amin(dim=-1)


def collapse(frame_pred, blank):
    """CTC greedy collapse of frame_pred [B, N] int64 (-1 beyond a clip's length): keep[t] = pred[t] != pred[t-1], pred[t] != blank and
    t inside the length -> (hyp_toks [B, N] left-packed and -1 filled, hyp_lens [B])."""
    B, N = frame_pred.shape
    hyp = torch.full((B, N), -1, dtype=torch.int64)
    lens = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        prev, n = -1, 0
        for t in range(N):
            cur = int(frame_pred[b, t])
            if cur >= 0 and cur != prev and cur != blank:
                hyp[b, n] = cur
                n += 1
            prev = cur
        lens[b] = n
    return hyp, lens


class Statement:
    def __init__(self, cfg, sd, dtype):
        self.cfg, self.dtype = cfg, dtype
        self.w = {k: v.to(dtype) for k, v in sd.items()}
        self.layers = []
        for l in range(cfg.num_layers):
            m = torch.nn.LSTM(cfg.embedding_dim if l == 0 else 2 * cfg.hidden_size, cfg.hidden_size, 1, batch_first=True, bidirectional=True).to(dtype)
            with torch.no_grad():
                for sfx in ("", "_reverse"):
                    for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                        getattr(m, f"{p}_l0{sfx}").copy_(self.w[f"encoder.rnn.{p}_l{l}{sfx}"])
            self.layers.append(m)

    def pooled(self, toks):
        """MultiHeadEmbedding, then the pooling, as the reference computes them."""
        cfg = self.cfg
        idx = toks + torch.arange(0, cfg.num_codebooks * cfg.vocab_size, cfg.vocab_size)
        if cfg.padding_idx:
            idx = torch.where(toks == cfg.vocab_size, torch.full_like(idx, cfg.num_codebooks * cfg.vocab_size), idx)
        x = self.w["embedding.weight"][idx]                                   # [B, N, K, E]
        if cfg.pooling == "linear":
            if cfg.num_codebooks == 1:
                return x[..., 0, :]
            return torch.nn.functional.linear(x.movedim(-1, -2), self.w["pooling.mlp.weight"])[..., 0]
        h = torch.relu(torch.nn.functional.linear(x, self.w["pooling.attn_mlp.0.weight"], self.w["pooling.attn_mlp.0.bias"]))
        attn = torch.softmax(torch.nn.functional.linear(h, self.w["pooling.attn_mlp.2.weight"]), dim=-2).squeeze(-1)   # [B, N, K]
        return (attn.unsqueeze(-2) @ x).movedim(-1, -2).squeeze(-1)

    @torch.no_grad()
    def forward(self, inp, lengths=None):
        """-> dict: pooled (with pooling), layer_out [layers, B, N, 2 H], logits, log_probs, and frame_pred, hyp_toks, hyp_lens (CTC) or
        pred (utterance).  `lengths`: a list of absolute frame counts or None."""
        cfg = self.cfg
        out = {}
        x = inp.to(self.dtype) if cfg.pooling is None else self.pooled(inp)
        if cfg.pooling is not None:
            out["pooled"] = x
        B, N = x.shape[0], x.shape[1]
        L = torch.full((B,), N, dtype=torch.int64) if lengths is None else torch.as_tensor(lengths, dtype=torch.int64).clamp(0, N)
        mask = torch.arange(N)[None, :] < L[:, None]
        ys = []
        for m in self.layers:
            pk = torch.nn.utils.rnn.pack_padded_sequence(x, L.clamp(min=1), batch_first=True, enforce_sorted=False)
            y = torch.nn.utils.rnn.pad_packed_sequence(m(pk)[0], batch_first=True, total_length=N)[0]
            x = y * mask[..., None]
            ys.append(x)
        out["layer_out"] = torch.stack(ys)
        if cfg.head == "ctc":
            logits = torch.nn.functional.linear(x, self.w["head.weight"], self.w["head.bias"])
            out["logits"] = logits
            out["log_probs"] = torch.log_softmax(logits, dim=-1) * mask[..., None]
            out["frame_pred"] = torch.where(mask, argmax_lowest(logits), torch.full((B, N), -1, dtype=torch.int64))
            out["hyp_toks"], out["hyp_lens"] = collapse(out["frame_pred"], cfg.blank_id)
        else:
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                stats = torch.stack([torch.cat([x[b, :int(L[b])].mean(dim=0), x[b, :int(L[b])].std(dim=0)]) for b in range(B)])
            logits = torch.nn.functional.linear(stats, self.w["head.weight"], self.w["head.bias"])
            out["logits"] = logits
            out["log_probs"] = torch.log_softmax(logits, dim=-1)
            out["pred"] = argmax_lowest(torch.nan_to_num(logits, nan=0.0))
        return out


def err(a, b):
    return float((a.double() - b.double()).abs().max())


def top2_gap(logits64):
    v = torch.topk(logits64, 2, dim=-1).values
    return v[..., 0] - v[..., 1]


def gap_rule(l64, l32):
    """bool: the rows whose fp64 arg-max is beyond doubt, by the fp32 statement's logit error on the same inputs."""
    return top2_gap(l64) > GAP_FACTOR * err(l32, l64)


_CASES = {}


def case(name):
    """The two statements on one case, computed once: dict(cfg, inp, lengths, s64, s32)."""
    if name not in _CASES:
        cname, B, N, lengths = CASES[name]
        cfg = CONFIGS[cname]
        inp = inputs(cfg, B, N)
        out = {"cfg": cfg, "inp": inp, "lengths": lengths}
        for dtype, tag in ((torch.float64, "s64"), (torch.float32, "s32")):
            out[tag] = Statement(cfg, weights(cfg), dtype).forward(inp, lengths)
        _CASES[name] = out
    return _CASES[name]


def valid_rows(c):
    """[B, N] bool for a CTC case: the frames inside the lengths."""
    B, N = c["inp"].shape[0], c["inp"].shape[1]
    return torch.arange(N)[None, :] < torch.as_tensor(c["lengths"])[:, None]
