"""tests/token_probe_ref.py (the statement of `TokenProbe`) against the reference's own embedding and pooling modules,
recorded in tests/golden/token_probe_ref.npz by tools/make_token_probe_golden.py; the folded attentional score table; the collapse against
`itertools.groupby`; every refusal that needs no GPU; and, for every shape of the GPU test, the frames the arg-max gap rule leaves out."""
import dataclasses
import itertools
import json
import os

import numpy as np
import pytest
import torch

import llama_score_ref
import token_probe_ref as PR
from audiocodecs_amd import PROBE_TINY, ProbeConfig, TokenProbe
from audiocodecs_amd.probe import check_config, fold_attn_scores, relative_to_frames, weight_names
from conftest import ROOT

GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "token_probe_ref.npz"))
META = json.loads(bytes(GOLDEN["meta_json"]).decode())
CTC_CASES = [n for n, (c, *_) in PR.CASES.items() if PR.CONFIGS[c].head == "ctc"]


def test_file_is_small_and_cap_is_the_projects():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "token_probe_ref.npz")) < 100 * 1024
    assert PR.CAP == llama_score_ref.CAP and PR.K_BOUND == llama_score_ref.K_BOUND and PR.GAP_FACTOR == llama_score_ref.GAP_FACTOR


@pytest.mark.parametrize("key", ["linear", "attentional_padded"])
def test_statement_agrees_with_the_reference(key):
    cfg = PR.CONFIGS[META["cases"][key]["config"]]
    toks = torch.from_numpy(GOLDEN[f"{key}_toks"].astype(np.int64))
    assert torch.equal(toks, PR.inputs(cfg, *toks.shape[:2]))
    assert META["cases"][key]["padded_ids"] == int((toks == cfg.vocab_size).sum()) and (META["cases"][key]["padded_ids"] > 0) == cfg.padding_idx
    gold = torch.from_numpy(GOLDEN[f"{key}_pooled"])
    p64 = PR.Statement(cfg, PR.weights(cfg), torch.float64).pooled(toks)
    p32 = PR.Statement(cfg, PR.weights(cfg), torch.float32).pooled(toks)
    bound = PR.K_BOUND * PR.err(p32, p64)
    e = PR.err(gold, p64)
    print(f"  {key}: pooled error of the reference {e:.3g}, bound {bound:.3g}")
    assert tuple(gold.shape) == tuple(p64.shape) and bound > 0.0 and e <= bound


def test_folded_scores_agree_with_the_mlp():
    cfg = PR.CONFIGS["TINY_ATT"]
    sd = {k: v.double() for k, v in PR.weights(cfg).items()}
    KC = cfg.num_codebooks * cfg.vocab_size
    table = fold_attn_scores(PR.weights(cfg)["embedding.weight"], PR.weights(cfg)["pooling.attn_mlp.0.weight"], PR.weights(cfg)["pooling.attn_mlp.0.bias"],
                             PR.weights(cfg)["pooling.attn_mlp.2.weight"], KC)
    mlp = lambda e: torch.relu(e @ sd["pooling.attn_mlp.0.weight"].T + sd["pooling.attn_mlp.0.bias"]) @ sd["pooling.attn_mlp.2.weight"][0]   # noqa: E731
    want = torch.cat([mlp(sd["embedding.weight"]), mlp(torch.zeros(1, cfg.embedding_dim, dtype=torch.float64))])
    assert table.dtype == torch.float32 and tuple(table.shape) == (KC + 2,)
    assert torch.equal(table, want.to(torch.float32))                         # rounded once
    # without a padding row the entry K C is a zero row's score
    plain = dataclasses.replace(cfg, padding_idx=False)
    t2 = fold_attn_scores(PR.weights(plain)["embedding.weight"], PR.weights(cfg)["pooling.attn_mlp.0.weight"], PR.weights(cfg)["pooling.attn_mlp.0.bias"],
                          PR.weights(cfg)["pooling.attn_mlp.2.weight"], KC)
    assert float(t2[KC]) == float(t2[KC + 1]) == float(table[KC + 1])


def test_collapse_agrees_with_groupby():
    g = torch.Generator().manual_seed(3)
    fp = torch.randint(0, 4, (6, 41), generator=g)
    lens = [41, 0, 1, 17, 40, 2]
    fp[0, 5:8] = torch.tensor([2, 0, 2])                                      # a repeated token across a blank stays twice
    fp[3, :17] = 0                                                            # decodes to nothing
    for b, n in enumerate(lens):
        fp[b, n:] = -1
    hyp, hl = PR.collapse(fp, 0)
    for b, n in enumerate(lens):
        want = [k for k, _ in itertools.groupby(fp[b, :n].tolist()) if k != 0]
        assert hyp[b, :int(hl[b])].tolist() == want and bool((hyp[b, int(hl[b]):] == -1).all())
    assert int(hl[1]) == 0 and int(hl[3]) == 0
    assert PR.collapse(torch.tensor([[2, 0, 2, 2, 1, -1]]), 0)[0].tolist() == [[2, 2, 1, -1, -1, -1]]


def test_statement_lengths_are_packed_sequences():
    """Backward starts at each clip's own last frame: a clip cut to L frames equals the clip of L frames alone; beyond L all is zero."""
    c = PR.case("tiny3")
    cfg, L = c["cfg"], c["lengths"][1]
    alone = PR.Statement(cfg, PR.weights(cfg), torch.float64).forward(c["inp"][1:2, :L])
    assert torch.equal(alone["layer_out"][:, 0], c["s64"]["layer_out"][:, 1, :L]) or PR.err(alone["layer_out"][:, 0], c["s64"]["layer_out"][:, 1, :L]) < 1e-14
    assert bool((c["s64"]["layer_out"][:, 1, L:] == 0).all()) and bool((c["s64"]["frame_pred"][1, L:] == -1).all())
    full = PR.Statement(cfg, PR.weights(cfg), torch.float64).forward(c["inp"])
    H = cfg.hidden_size                                                       # (clip 2 has one frame: t = 0 is where its backward pass starts)
    assert PR.err(full["layer_out"][0, 2, 0, H:], c["s64"]["layer_out"][0, 2, 0, H:]) > 1e-2
    assert PR.err(full["layer_out"][0, 1, 0, H:], c["s64"]["layer_out"][0, 1, 0, H:]) > 1e-5


def test_utterance_statement_nan_conventions():
    cfg = PR.CONFIGS["TINY_UTT"]
    out = PR.Statement(cfg, PR.weights(cfg), torch.float64).forward(PR.inputs(cfg, 3, 9), [9, 1, 0])
    assert bool(torch.isfinite(out["log_probs"][0]).all()) and bool(torch.isnan(out["log_probs"][1]).all()) and bool(torch.isnan(out["log_probs"][2]).all())


@pytest.mark.parametrize("name", CTC_CASES)
def test_gap_rule_stays_inside_the_cap(name):
    """The frames whose arg-max the gap rule does not decide are counted; the fp32 statement agrees with fp64 on all the others."""
    c = PR.case(name)
    valid = PR.valid_rows(c)
    sure = PR.gap_rule(c["s64"]["logits"], c["s32"]["logits"])
    out = int((~sure & valid).sum())
    print(f"  {name}: {out} of {int(valid.sum())} frames inside the gap")
    assert out <= PR.CAP * int(valid.sum())
    assert torch.equal(c["s32"]["frame_pred"][sure], c["s64"]["frame_pred"][sure])


@pytest.mark.parametrize("name", [n for n in PR.CASES if n not in CTC_CASES])
def test_gap_rule_of_the_utterance_cases(name):
    c = PR.case(name)
    sure = PR.gap_rule(c["s64"]["logits"], c["s32"]["logits"])
    print(f"  {name}: {int((~sure).sum())} of {sure.numel()} clips inside the gap")
    assert bool(sure.all()) and torch.equal(c["s32"]["pred"], c["s64"]["pred"])


def test_ctc_cases_hold_the_patterns_the_gpu_test_needs():
    """A repeated token across a blank (tiny3, tiny35) and a clip that decodes to nothing (tiny35's clips of length 0)."""
    for name in ("tiny3", "tiny35"):
        fp = PR.case(name)["s64"]["frame_pred"]
        assert any(r[t] > 0 and r[t - 1] == 0 and r[t - 2] == r[t] for r in fp.tolist() for t in range(2, len(r))), name
    c = PR.case("tiny35")
    assert 0 in c["lengths"] and int(c["s64"]["hyp_lens"][c["lengths"].index(0)]) == 0


def test_refusals_without_a_gpu():
    sd = PR.weights(PROBE_TINY)
    with pytest.raises(NotImplementedError, match="list-valued"):
        check_config(dataclasses.replace(PROBE_TINY, vocab_size=[50, 50]))
    with pytest.raises(ValueError, match="multiple of 32"):
        TokenProbe(state_dict=sd, config=dataclasses.replace(PROBE_TINY, hidden_size=48))
    with pytest.raises(ValueError, match="no recurrence kernel"):
        TokenProbe(state_dict=sd, config=dataclasses.replace(PROBE_TINY, hidden_size=96))
    with pytest.raises(ValueError, match="matrix pipe"):
        TokenProbe(state_dict=sd, config=dataclasses.replace(PROBE_TINY, embedding_dim=24))
    with pytest.raises(ValueError, match="exact-product"):
        TokenProbe(state_dict=sd, config=PROBE_TINY, precision="fp32_exact")
    with pytest.raises(ValueError, match="pooling"):
        check_config(dataclasses.replace(PROBE_TINY, pooling="weighted"))
    with pytest.raises(ValueError, match="head"):
        check_config(dataclasses.replace(PROBE_TINY, head="frames"))
    with pytest.raises(ValueError, match="blank_id"):
        check_config(dataclasses.replace(PROBE_TINY, blank_id=11))
    with pytest.raises(KeyError, match="lacks"):
        TokenProbe(state_dict={k: v for k, v in sd.items() if k != "head.bias"}, config=PROBE_TINY)
    with pytest.raises(ValueError, match="head.weight"):
        TokenProbe(state_dict={**sd, "head.weight": sd["head.weight"][:, :64]}, config=PROBE_TINY)
    probe = TokenProbe(state_dict=sd, config=PROBE_TINY)
    with pytest.raises(ValueError, match="integer dtype"):
        probe.forward(torch.zeros(2, 5, 2))
    with pytest.raises(ValueError, match="integer dtype"):
        probe.forward(torch.zeros(2, 5, 3, dtype=torch.int64))
    with pytest.raises(Exception, match="no CPU fallback"):
        probe.forward(torch.zeros(2, 5, 2, dtype=torch.int64))
    assert weight_names(PR.CONFIGS["TINY_ATT"])[1:4] == ["pooling.attn_mlp.0.weight", "pooling.attn_mlp.0.bias", "pooling.attn_mlp.2.weight"]
    assert isinstance(PROBE_TINY, ProbeConfig) and (PROBE_TINY.hidden_size, PROBE_TINY.embedding_dim, PROBE_TINY.num_codebooks, PROBE_TINY.vocab_size) == (64, 32, 2, 50)


def test_relative_lengths_round_to_frames():
    assert relative_to_frames(torch.tensor([1.0, 0.5, 0.26, 0.0]), 37).tolist() == [37, 18, 10, 0]
