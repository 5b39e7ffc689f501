"""tests/llama_score_ref.py (the statement of `LlamaDecoder.score`) against the reference's own decoder, recorded
in tests/golden/llama_score_ref.npz by tools/make_llama_score_golden.py; the `input_dim` fold; and every refusal of `score` that needs no
GPU.  The GPU test's shapes are held to the gap rule's cap here too: the seeds are chosen so that the fp32 statement alone stays inside it."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

import llama_ref as R
import llama_score_ref as SR
from audiocodecs_amd import IGNORE, LlamaDecoder, LlamaScore
from audiocodecs_amd.llama import fold_input, weight_names
from conftest import ROOT

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "llama_score_ref.npz"))
META = json.loads(bytes(GOLDEN["meta_json"]).decode())
# every shape a test scores: the golden file's and the GPU test's (tests/test_llama_score_gpu.py)
SHAPES = [(n, *SR.GOLDEN_SHAPE) for n in SR.CONFIGS if n != "TINY_HD128"] + [(n, 1, 6, 201) for n in SR.CONFIGS if n != "TINY_HD128"] + \
         [("TINY_HD128", *SR.GOLDEN_SHAPE), ("TINY_HD128", 3, 6, 131), ("TINY_HD128", 1, 6, 131), ("TINY", 2, 0, 1000)]


@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_statement_agrees_with_the_reference(name):
    B, P, T = SR.GOLDEN_SHAPE
    c = SR.case(name, B, P, T)
    assert META["cases"][name]["P"] == (P if SR.CONFIGS[name].prompt_dim else 0)
    assert np.array_equal(GOLDEN[f"{name}_toks"], c["toks"].numpy()) and np.array_equal(GOLDEN[f"{name}_targets"], c["targets"].numpy())
    assert int((c["targets"] == IGNORE).sum()) > 0 and META["cases"][name]["scored"] == int(c["s64"]["count"].sum())
    gold = torch.from_numpy(GOLDEN[f"{name}_logp"])
    bound = SR.K_BOUND * R.err(c["s32"]["logp"], c["s64"]["logp"])
    e = R.err(gold, c["s64"]["logp"])
    print(f"  {name}: log-prob error of the reference {e:.3g}, bound {bound:.3g}")
    assert bound > 0.0 and e <= bound
    assert bool((gold[c["targets"] == IGNORE] == 0).all()) and bool((c["s64"]["logp"][c["targets"] == IGNORE] == 0).all())
    sure = SR.gap_rule(c["l64"], c["l32"])
    pred = torch.from_numpy(GOLDEN[f"{name}_pred"].astype(np.int64))
    assert torch.equal(pred[sure], c["s64"]["pred"][sure])


@pytest.mark.parametrize("name,B,P,T", SHAPES)
def test_gap_rule_stays_inside_the_cap(name, B, P, T):
    """The positions whose arg-max the gap rule does not decide are counted; the fp32 statement agrees with fp64 on all the others."""
    c = SR.case(name, B, P, T)
    sure = SR.gap_rule(c["l64"], c["l32"])
    out = int((~sure).sum())
    print(f"  {name} B={B} T={T}: {out} of {sure.numel()} positions inside the gap")
    assert out <= SR.CAP * sure.numel()
    assert torch.equal(c["s32"]["pred"][sure], c["s64"]["pred"][sure])


def test_score_statement_masks_and_sums():
    logits = torch.tensor([[[0.0, 2.0, 2.0, -1.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 3.0]]], dtype=torch.float64)
    targets = torch.tensor([[2, IGNORE, 3]])
    s = SR.score(logits, targets)
    assert s["pred"].tolist() == [[1, 0, 3]]                                  # the lowest index of the two equal maxima
    lp = torch.log_softmax(logits, dim=-1)
    assert s["logp"][0, 1] == 0 and s["logp"][0, 0] == lp[0, 0, 2] and int(s["count"]) == 2 and int(s["errors"]) == 1
    assert float(s["sum_logp"]) == float(lp[0, 0, 2] + lp[0, 2, 3])
    cut = SR.score(logits, torch.tensor([[2, 0, 7]]), lengths=[1])            # 7: outside the vocabulary; length 1: position 0 alone
    assert int(cut["count"]) == 1 and cut["logp"][0, 1:].abs().sum() == 0
    r = LlamaScore(s["logp"], s["pred"], s["sum_logp"], s["count"], s["errors"])
    assert float(r.nll) == -float(s["sum_logp"]) / 2 and float(r.ter) == 0.5 and float(r.mean_logp[0]) == float(s["sum_logp"]) / 2


def test_input_dim_fold():
    cfg = SR.TINY_IN
    sd = SR.weights(cfg)
    assert "input.weight" in weight_names(cfg) and "input.weight" not in weight_names(R.TINY)
    assert tuple(sd["tok_embeddings.weight"].shape) == (cfg.num_codebooks * cfg.vocab_size, cfg.input_dim)
    folded = fold_input(sd["tok_embeddings.weight"], sd["input.weight"])
    exact = sd["tok_embeddings.weight"].double() @ sd["input.weight"].double().T
    assert folded.dtype == torch.float32 and torch.equal(folded, exact.float())                  # rounded once
    dec = LlamaDecoder(state_dict=sd, config=cfg)
    assert torch.equal(dec._weights["tok_embeddings.weight"], folded) and "input.weight" not in dec._weights
    toks, _, _ = SR.inputs(cfg, 2, 0, 9)
    s = SR.Statement(cfg, sd, torch.float64)
    k = torch.arange(9) % cfg.num_codebooks
    assert R.err(folded[toks + k * cfg.vocab_size], s.embed(toks)) <= 2.0 ** -24 * float(exact.abs().max())
    with pytest.raises(KeyError):
        LlamaDecoder(state_dict={k: v for k, v in sd.items() if k != "input.weight"}, config=cfg)
    with pytest.raises(ValueError):
        LlamaDecoder(state_dict=sd, config=dataclasses.replace(cfg, input_dim=16))
    plain = LlamaDecoder(state_dict=R.weights(R.TINY), config=R.TINY)                            # input_dim=None: the table is the caller's
    assert plain._weights["tok_embeddings.weight"] is R.weights(R.TINY)["tok_embeddings.weight"]


def test_refusals_without_a_gpu():
    cfg = R.TINY
    dec = LlamaDecoder(state_dict=R.weights(cfg), config=cfg)
    toks = torch.zeros(2, 8, dtype=torch.int64)
    tg = torch.zeros(2, 8, dtype=torch.int64)
    bad = [
        dict(toks=toks.float(), targets=tg), dict(toks=toks[0], targets=tg), dict(toks=toks, targets=tg.int()), dict(toks=toks, targets=tg[:, :7]),
        dict(toks=toks, targets=tg[:1]), dict(toks=toks[:, :0], targets=tg[:, :0]),
        dict(toks=toks, targets=tg, prompt_embs=torch.zeros(2, 3, cfg.prompt_dim)),                          # 3 rows: no multiple of 2 codebooks
        dict(toks=toks, targets=tg, prompt_embs=torch.zeros(3, 2, cfg.prompt_dim)), dict(toks=toks, targets=tg, prompt_embs=torch.zeros(2, 2, cfg.prompt_dim).double()),
        dict(toks=torch.zeros(1, 2 * cfg.max_seq_len + 1, dtype=torch.int64), targets=torch.zeros(1, 2 * cfg.max_seq_len + 1, dtype=torch.int64)),
        dict(toks=torch.zeros(1, 2 * cfg.max_seq_len - 1, dtype=torch.int64), targets=torch.zeros(1, 2 * cfg.max_seq_len - 1, dtype=torch.int64),
             prompt_embs=torch.zeros(1, 2, cfg.prompt_dim)),
        dict(toks=toks, targets=tg, lengths=[9, 0]), dict(toks=toks, targets=tg, lengths=[-1, 0]), dict(toks=toks, targets=tg, lengths=[1]),
        dict(toks=toks, targets=tg, lengths=torch.tensor([1.0, 2.0])), dict(toks=toks, targets=tg, lengths=torch.tensor([8, 9])),
        dict(toks=toks, targets=tg, lengths=[1, True]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            dec.score(kw.pop("toks"), kw.pop("targets"), **kw)
    with pytest.raises(Exception) as e:                     # everything fits: the refusal is the missing device, not a ValueError
        dec.score(toks, tg, lengths=[8, 0])
    assert not isinstance(e.value, ValueError)
