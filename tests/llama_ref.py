"""The statement of the Llama decoder (audiocodecs_amd.llama) in torch, parameterised by dtype, the synthetic
weights and the configurations that the CPU tests, the GPU tests and tools/llama_latency.py share.

fp64 is the yardstick; the same statement in fp32 on the CPU supplies each bound: a tensor of the library may differ from the fp64
statement by at most K = 8 times what the fp32 statement differs from it on the same inputs (the project's factor, tests/test_spksim_gpu.py).

Semantics: RMSNorm x * rsqrt(mean(x^2) + eps) * w; wq | wk | wv without bias; RoPE on the interleaved pairs (2i, 2i + 1) of q and k by
row `pos` of the fp32 table (data: the statement casts it, it does not recompute an angle); causal attention scaled by 1 / sqrt(head_dim),
query head h reading key/value head h // (n_heads // n_kv_heads); wo plus residual; RMSNorm, w2(silu(w1 x) * w3 x) plus residual; the
final RMSNorm and, at absolute position p, output head p % num_codebooks.  Token j of `embed(toks, curr_pos)` reads table row
tok + ((curr_pos + j) % num_codebooks) * vocab_size.
"""
import numpy as np
import torch

from audiocodecs_amd import prng
from audiocodecs_amd.llama import LlamaConfig, rope_table, weight_names

K_BOUND = 8.0
GAP_FACTOR = 16.0
W_SCALE = 3.0      # matrix weights: W_SCALE times a normal of nn.Linear's default variance 1 / (3 fan_in): logits with a spread near 1.7

TINY = LlamaConfig(vocab_size=130, n_layers=2, dim=64, ffn_dim=128, n_heads=4, n_kv_heads=1, max_seq_len=512, prompt_dim=24, num_codebooks=2)
TINY_G2 = LlamaConfig(vocab_size=130, n_layers=1, dim=64, ffn_dim=128, n_heads=4, n_kv_heads=2, max_seq_len=512, prompt_dim=None, num_codebooks=1)
TINY_HD128 = LlamaConfig(vocab_size=1026, n_layers=1, dim=256, ffn_dim=512, n_heads=2, n_kv_heads=1, max_seq_len=512, prompt_dim=24, num_codebooks=2)
CONFIGS = {"TINY": TINY, "TINY_G2": TINY_G2, "TINY_HD128": TINY_HD128}

_WEIGHTS = {}


def _shape(cfg, name):
    hd, d, f = cfg.head_dim, cfg.dim, cfg.ffn
    if name == "tok_embeddings.weight":
        return (cfg.num_codebooks * cfg.vocab_size, d)
    if name == "prompt.weight":
        return (d, cfg.prompt_dim)
    if name.startswith("output"):
        return (cfg.vocab_size, d)
    if name.endswith("norm.weight"):
        return (d,)
    leaf = name.split(".")[-2]
    return {"wq": (cfg.n_heads * hd, d), "wk": (cfg.n_kv_heads * hd, d), "wv": (cfg.n_kv_heads * hd, d), "wo": (d, cfg.n_heads * hd),
            "w1": (f, d), "w3": (f, d), "w2": (d, f)}[leaf]


def weights(cfg, seed=0):
    """The synthetic state dict of `cfg` (fp32 CPU tensors, the reference's keys), from the repository's PRNG; computed once."""
    key = (cfg, seed)
    if key not in _WEIGHTS:
        sd = {}
        for name in weight_names(cfg):
            shape = _shape(cfg, name)
            x = prng.normal(seed, "llama." + name, shape)
            if len(shape) == 1:
                x = 1.0 + 0.1 * x
            elif name != "tok_embeddings.weight":
                x = x * (W_SCALE / np.sqrt(3.0 * shape[1]))
            sd[name] = torch.from_numpy(x.astype(np.float32))
        _WEIGHTS[key] = sd
    return _WEIGHTS[key]


def inputs(cfg, B, P, T, seed=1):
    """(bos / text tokens [B, T] int64, prompt [B, P, prompt_dim] fp32 or None)."""
    toks = torch.from_numpy(prng.randint(seed, "llama.toks", [B, T], cfg.vocab_size))
    prompt = torch.from_numpy(prng.normal(seed, "llama.prompt", [B, P, cfg.prompt_dim]).astype(np.float32)) if P and cfg.prompt_dim else None
    return toks, prompt


class Statement:
    """The decoder in `dtype` on `device`, with a KV cache: allocated once for `capacity` positions and written in place, or, without
    a capacity, grown by concatenation."""

    def __init__(self, cfg, sd, dtype=torch.float64, device="cpu", wrong_grouping=False, capacity=None):
        self.cfg, self.dtype, self.device = cfg, dtype, torch.device(device)
        self.w = {k: v.to(device=self.device, dtype=dtype) for k, v in sd.items()}
        cos, sin = rope_table(cfg)
        self.cos, self.sin = cos.to(device=self.device, dtype=dtype), sin.to(device=self.device, dtype=dtype)
        self.wrong_grouping, self.capacity = wrong_grouping, capacity
        self.reset()

    def reset(self):
        self.pos, self.kv = 0, [None] * self.cfg.n_layers

    def embed(self, toks, prompt_embs=None, curr_pos=0):
        cfg = self.cfg
        toks = toks.to(self.device)
        k = (curr_pos + torch.arange(toks.shape[1], device=self.device)) % cfg.num_codebooks
        embs = self.w["tok_embeddings.weight"][toks + k * cfg.vocab_size]
        if prompt_embs is not None:
            p = prompt_embs.to(device=self.device, dtype=self.dtype)
            if cfg.prompt_dim is not None and p.shape[-1] == cfg.prompt_dim:
                p = p @ self.w["prompt.weight"].T
            embs = torch.cat([p, embs], dim=1)
        return embs

    def _norm(self, x, w):
        return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + self.cfg.norm_eps) * w

    def _rope(self, x, pos0):
        T = x.shape[1]
        c, s = self.cos[pos0:pos0 + T][None, :, None, :], self.sin[pos0:pos0 + T][None, :, None, :]
        a, b = x[..., 0::2], x[..., 1::2]
        return torch.stack([a * c - b * s, a * s + b * c], dim=-1).flatten(-2)

    def forward(self, embs, stages=None):
        """embs [B, T, dim] appended at self.pos -> logits [B, T, C]; `stages`: a dict that receives per layer "q", "k", "attn",
        "layer_out" (lists) and "final_norm"."""
        cfg, w = self.cfg, self.w
        x = embs.to(device=self.device, dtype=self.dtype)
        B, T, _ = x.shape
        hd, nh, nkv, pos0 = cfg.head_dim, cfg.n_heads, cfg.n_kv_heads, self.pos
        for l in range(cfg.n_layers):
            p = f"layers.{l}."
            h = self._norm(x, w[p + "attention_norm.weight"])
            q = self._rope((h @ w[p + "attention.wq.weight"].T).view(B, T, nh, hd), pos0)
            k = self._rope((h @ w[p + "attention.wk.weight"].T).view(B, T, nkv, hd), pos0)
            v = (h @ w[p + "attention.wv.weight"].T).view(B, T, nkv, hd)
            if self.capacity:
                if self.kv[l] is None:
                    self.kv[l] = (x.new_zeros(B, self.capacity, nkv, hd), x.new_zeros(B, self.capacity, nkv, hd))
                self.kv[l][0][:, pos0:pos0 + T], self.kv[l][1][:, pos0:pos0 + T] = k, v
                k, v = self.kv[l][0][:, :pos0 + T], self.kv[l][1][:, :pos0 + T]
            else:
                if self.kv[l] is not None:
                    k, v = torch.cat([self.kv[l][0], k], dim=1), torch.cat([self.kv[l][1], v], dim=1)
                self.kv[l] = (k, v)
            S = k.shape[1]
            head_of = torch.arange(nh, device=self.device) % nkv if self.wrong_grouping else torch.arange(nh, device=self.device) // (nh // nkv)
            kk, vv = k[:, :, head_of], v[:, :, head_of]                                      # [B, S, nh, hd]
            sc = torch.einsum("bthd,bshd->bhts", q, kk) / (hd ** 0.5)
            causal = torch.arange(S, device=self.device)[None, :] > (pos0 + torch.arange(T, device=self.device))[:, None]
            sc = sc.masked_fill(causal[None, None], float("-inf"))
            att = torch.einsum("bhts,bshd->bthd", torch.softmax(sc, dim=-1), vv).reshape(B, T, nh * hd)
            x = x + att @ w[p + "attention.wo.weight"].T
            h = self._norm(x, w[p + "ffn_norm.weight"])
            x = x + (torch.nn.functional.silu(h @ w[p + "feed_forward.w1.weight"].T) * (h @ w[p + "feed_forward.w3.weight"].T)) @ w[p + "feed_forward.w2.weight"].T
            if stages is not None:
                stages.setdefault("q", []).append(q.reshape(B, T, nh * hd))
                stages.setdefault("k", []).append(k[:, pos0:pos0 + T])
                stages.setdefault("attn", []).append(att)
                stages.setdefault("layer_out", []).append(x)
        x = self._norm(x, w["norm.weight"])
        if stages is not None:
            stages["final_norm"] = x
        if cfg.num_codebooks > 1:
            heads = torch.stack([w[f"output.{k}.weight"] for k in range(cfg.num_codebooks)])           # [K, C, dim]
            which = (pos0 + torch.arange(T, device=self.device)) % cfg.num_codebooks
            logits = torch.einsum("btd,tcd->btc", x, heads[which])
        else:
            logits = x @ w["output.weight"].T
        self.pos = pos0 + T
        return logits

    def generate_greedy(self, bos_toks, eos_id, prompt_embs=None, max_gen_toks=100):
        """The reference's loop at top_p = 0 -> (list of rows hyp[i, :lens[i]], the [steps, B, C] logits of every step)."""
        self.reset()
        B = bos_toks.shape[0]
        embs = self.embed(bos_toks, prompt_embs)
        hyp = torch.full((B, max_gen_toks), eos_id, dtype=torch.int64)
        lens, alive, log, n = torch.zeros(B, dtype=torch.int64), torch.ones(B, dtype=torch.bool), [], 0
        while n < max_gen_toks:
            logits = self.forward(embs)[:, -1]
            log.append(logits.cpu())
            tok = logits.argmax(dim=-1).cpu()
            hyp[:, n] = tok
            alive &= tok != eos_id
            lens[alive] += 1
            n += 1
            if not alive.any():
                break
            embs = self.embed(tok[:, None], curr_pos=n)
        return [hyp[i, :lens[i]] for i in range(B)], torch.stack(log)


def lens_of(hyp, eos_id):
    """The reference's `lens` on recorded tokens hyp [B, steps]: a row counts its tokens before its first EOS."""
    out = []
    for row in hyp.tolist():
        out.append(row.index(eos_id) if eos_id in row else len(row))
    return out


def err(a, b):
    return float((a.double() - b.double()).abs().max())


def top2_gap(logits64):
    v = torch.topk(logits64, 2, dim=-1).values
    return v[..., 0] - v[..., 1]
