"""The statement of `LlamaDecoder.score` (audiocodecs_amd.llama) in torch, by dtype, on top of tests/llama_ref.py:
the decoder with the ``input`` Linear behind its embedding table (`TINY_IN`), and the scoring rule -- log_softmax, the target's
log-probability, the arg-max with the lowest index on a tie, and the sums under the masking rules.  Shared by the CPU test, the GPU test,
tools/make_llama_score_golden.py and tools/llama_score_latency.py.

fp64 is the yardstick and the same statement in fp32 supplies each bound, as in llama_ref: K_BOUND times its error for a tensor; an arg-max
has to agree wherever the fp64 top-two gap exceeds GAP_FACTOR times the fp32 statement's logit error, and the positions that rule leaves out
are counted against CAP.
"""
import dataclasses

import numpy as np
import torch

import llama_ref as R
from audiocodecs_amd import prng
from audiocodecs_amd.llama import IGNORE

K_BOUND, GAP_FACTOR = R.K_BOUND, R.GAP_FACTOR
CAP = 0.03         # the share of positions the gap rule may leave out (sampling_ref's cap)

TINY_IN = dataclasses.replace(R.TINY, input_dim=24)
CONFIGS = {**R.CONFIGS, "TINY_IN": TINY_IN}

# the cases of the golden file and of the GPU test: (B, P with a prompt, T); P is 0 for a configuration without prompt_dim
GOLDEN_SHAPE = (3, 6, 201)

_WEIGHTS = {}


def weights(cfg, seed=0):
    """llama_ref's synthetic state dict; with `input_dim` the table has that width and "input.weight" [dim, input_dim] follows it."""
    if cfg.input_dim is None:
        return R.weights(cfg, seed)
    key = (cfg, seed)
    if key not in _WEIGHTS:
        sd = dict(R.weights(dataclasses.replace(cfg, input_dim=None), seed))
        sd["tok_embeddings.weight"] = torch.from_numpy(prng.normal(seed, "llama.tok_embeddings.in", (cfg.num_codebooks * cfg.vocab_size, cfg.input_dim)).astype(np.float32))
        w = prng.normal(seed, "llama.input.weight", (cfg.dim, cfg.input_dim)) * (R.W_SCALE / np.sqrt(3.0 * cfg.input_dim))
        sd["input.weight"] = torch.from_numpy(w.astype(np.float32))
        _WEIGHTS[key] = sd
    return _WEIGHTS[key]


def inputs(cfg, B, P, T, seed=1):
    """(toks [B, T], prompt [B, P, prompt_dim] or None, targets [B, T] int64 with a few IGNORE)."""
    toks, prompt = R.inputs(cfg, B, P, T, seed)
    targets = torch.from_numpy(prng.randint(seed, "llama.targets", [B, T], cfg.vocab_size))
    drop = torch.from_numpy(prng.randint(seed, "llama.targets.ignore", [B, T], 16)) == 0
    return toks, prompt, torch.where(drop, torch.full_like(targets, IGNORE), targets)


class Statement(R.Statement):
    """llama_ref's decoder whose `embed` runs the unfolded ``input`` Linear when the configuration has one."""

    def embed(self, toks, prompt_embs=None, curr_pos=0):
        cfg = self.cfg
        if cfg.input_dim is None:
            return super().embed(toks, prompt_embs, curr_pos)
        toks = toks.to(self.device)
        k = (curr_pos + torch.arange(toks.shape[1], device=self.device)) % cfg.num_codebooks
        embs = self.w["tok_embeddings.weight"][toks + k * cfg.vocab_size] @ self.w["input.weight"].T
        if prompt_embs is not None:
            p = prompt_embs.to(device=self.device, dtype=self.dtype)
            if cfg.prompt_dim is not None and p.shape[-1] == cfg.prompt_dim:
                p = p @ self.w["prompt.weight"].T
            embs = torch.cat([p, embs], dim=1)
        return embs

    def token_logits(self, toks, prompt_embs=None, stages=None):
        """The logits [B, T, C] of the token rows of one forward over [prompt | toks] from position 0."""
        self.reset()
        P = 0 if prompt_embs is None else prompt_embs.shape[1]
        return self.forward(self.embed(toks, prompt_embs), stages)[:, P:]


def scored_mask(targets, vocab, lengths=None):
    T = targets.shape[1]
    m = (targets >= 0) & (targets < vocab)
    if lengths is not None:
        m = m & (torch.arange(T, device=targets.device)[None, :] < torch.as_tensor(lengths, device=targets.device)[:, None])
    return m


def argmax_lowest(logits):
    """The arg-max with the lowest index on a tie."""
    C = logits.shape[-1]
    idx = torch.arange(C, device=logits.device).expand_as(logits)
    return torch.where(logits == logits.amax(dim=-1, keepdim=True), idx, torch.full_like(idx, C)).amin(dim=-1)


def score(logits, targets, lengths=None):
    """The scoring rule on logits [B, T, C] of any dtype -> dict(logp [B, T] in that dtype, pred, sum_logp fp64, count, errors)."""
    C = logits.shape[-1]
    targets = targets.to(logits.device)
    m = scored_mask(targets, C, lengths)
    lp = torch.log_softmax(logits, dim=-1).gather(-1, targets.clamp(0, C - 1)[..., None])[..., 0]
    logp = torch.where(m, lp, torch.zeros_like(lp))
    pred = argmax_lowest(logits)
    return {"logp": logp, "pred": pred, "sum_logp": logp.double().sum(dim=-1), "count": m.sum(dim=-1), "errors": (m & (pred != targets)).sum(dim=-1)}


def gap_rule(l64, l32):
    """[B, T] bool: the positions whose fp64 arg-max is beyond doubt, by the fp32 statement's logit error on the same inputs."""
    return R.top2_gap(l64) > GAP_FACTOR * R.err(l32, l64)


_CASES = {}


def case(name, B, P, T, stages=False):
    """The two statements on one shape, computed once: dict(toks, prompt, targets, l64, l32, s64, s32 [, g64, g32: the stage dicts])."""
    key = (name, B, P, T, stages)
    if key not in _CASES:
        cfg = CONFIGS[name]
        toks, prompt, targets = inputs(cfg, B, P if cfg.prompt_dim else 0, T)
        out = {"toks": toks, "prompt": prompt, "targets": targets}
        for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
            s = Statement(cfg, weights(cfg), dtype)
            g = {} if stages else None
            out["e" + tag] = s.embed(toks, prompt)
            out["l" + tag] = s.token_logits(toks, prompt, g)
            out["s" + tag] = score(out["l" + tag], targets)
            if stages:
                out["g" + tag] = g
        _CASES[key] = out
    return _CASES[key]
