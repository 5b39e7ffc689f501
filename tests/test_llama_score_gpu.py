"""`LlamaDecoder.score` on the GPU (audiocodecs_amd.llama) against tests/llama_score_ref.py.  The bound of a tensor
is K_BOUND = 8 times the error of the fp32 statement against the fp64 statement on the same inputs, computed here (llama_score_ref.case),
never from the library's output -- the rule of tests/test_llama_gpu.py.  Shapes: 6 + 201 = 207 rows cross the 64- and 128-row tile seams
of the GEMM, are no multiple of the attention's 16 queries and leave a ragged last tile; 1000 rows lie beyond max_seq_len, inside the rotary
table, and walk sixteen key tiles."""
import pytest
import torch

import llama_ref as R
import llama_score_ref as SR
from audiocodecs_amd import IGNORE, LlamaDecoder, LlamaScore

pytestmark = pytest.mark.gpu

_DEC, _RUNS = {}, {}


def decoder(name):
    if name not in _DEC:
        _DEC[name] = LlamaDecoder(state_dict=SR.weights(SR.CONFIGS[name]), config=SR.CONFIGS[name])
    return _DEC[name]


def gpu_inputs(name, B, P, T):
    c = SR.case(name, B, P, T, stages=True)
    return c, c["toks"].cuda(), c["targets"].cuda(), None if c["prompt"] is None else c["prompt"].cuda()


def run(name, B, P, T):
    """One `score(..., return_stages=True)` per shape."""
    key = (name, B, P, T)
    if key not in _RUNS:
        _, toks, targets, prompt = gpu_inputs(name, B, P, T)
        _RUNS[key] = decoder(name).score(toks, targets, prompt_embs=prompt, return_stages=True)
    return _RUNS[key]


def check(what, got, s64, s32):
    bound = SR.K_BOUND * R.err(s32, s64)
    e = R.err(got.cpu(), s64)
    print(f"  {what}: error {e:.3g}, bound {bound:.3g}")
    assert tuple(got.shape) == tuple(s64.shape), what
    assert bound > 0.0 and e <= bound, (what, e, bound)
    return bound


def check_pred(what, out, c):
    """`pred` is the arg-max of the returned logits exactly, and the fp64 arg-max wherever the gap rule decides."""
    assert torch.equal(out.pred, SR.argmax_lowest(out.stages["logits"])), what
    sure = SR.gap_rule(c["l64"], c["l32"])
    left = int((~sure).sum())
    print(f"  {what}: {left} of {sure.numel()} positions inside the gap")
    assert left <= SR.CAP * sure.numel()
    assert torch.equal(out.pred.cpu()[sure], c["s64"]["pred"][sure]), what


def same(a: LlamaScore, b: LlamaScore, rows=slice(None)):
    return all(torch.equal(getattr(a, f)[rows], getattr(b, f)) for f in ("logp", "pred", "sum_logp", "count", "errors"))


def test_score_exists_and_returns_the_fields():
    """Fails without the feature: the method, the result type and the ignore id are new."""
    import audiocodecs_amd as A

    assert A.IGNORE == -1 and A.LlamaScore is LlamaScore and hasattr(A.llama.LlamaConfig(), "input_dim")
    B, T = 2, 9
    _, toks, targets, prompt = gpu_inputs("TINY", B, 6, T)
    out = decoder("TINY").score(toks, targets, prompt_embs=prompt)
    assert isinstance(out, LlamaScore) and out.stages is None
    want = {"logp": ((B, T), torch.float32), "pred": ((B, T), torch.int64), "sum_logp": ((B,), torch.float64), "count": ((B,), torch.int64), "errors": ((B,), torch.int64)}
    for f, (shape, dtype) in want.items():
        t = getattr(out, f)
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == dtype, f
    assert torch.isfinite(out.nll) and 0.0 <= float(out.ter) <= 1.0 and tuple(out.mean_logp.shape) == (B,)


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("name", list(SR.CONFIGS))
def test_stages_and_log_probs(name, B):
    cfg = SR.CONFIGS[name]
    P, T = 6, 131 if name == "TINY_HD128" else 201
    c, toks, targets, prompt = gpu_inputs(name, B, P, T)
    out = run(name, B, P, T)
    st, g64, g32 = out.stages, c["g64"], c["g32"]
    Ttot = T + (P if prompt is not None else 0)
    embs = decoder(name).embed(toks, prompt)
    if prompt is not None or cfg.input_dim is not None:
        check("embed", embs, c["e64"], c["e32"])
    else:
        assert torch.equal(embs.cpu().double(), c["e64"])
    for l in range(cfg.n_layers):
        check(f"q[{l}]", st["q"][l], g64["q"][l], g32["q"][l])
        check(f"k[{l}]", st["k"][l], g64["k"][l].reshape(B, Ttot, -1), g32["k"][l].reshape(B, Ttot, -1))
        check(f"attn[{l}]", st["attn"][l], g64["attn"][l], g32["attn"][l])
        check(f"layer_out[{l}]", st["layer_out"][l], g64["layer_out"][l], g32["layer_out"][l])
    check("final_norm", st["final_norm"], g64["final_norm"], g32["final_norm"])
    bound = check("logits", st["logits"], c["l64"], c["l32"])
    check("logp", out.logp, c["s64"]["logp"], c["s32"]["logp"])
    check_pred(name, out, c)
    if name == "TINY_G2":
        w = SR.Statement(cfg, SR.weights(cfg), torch.float64, wrong_grouping=True)
        assert R.err(st["logits"].cpu(), w.token_logits(c["toks"], c["prompt"])) > bound


def test_beyond_max_seq_len():
    name, B, P, T = "TINY", 2, 0, 1000
    assert T > SR.CONFIGS[name].max_seq_len
    c, _, _, _ = gpu_inputs(name, B, P, T)
    out = run(name, B, P, T)
    check("logits", out.stages["logits"], c["l64"], c["l32"])
    check("logp", out.logp, c["s64"]["logp"], c["s32"]["logp"])
    check_pred(name, out, c)


def test_equal_maxima_take_the_lowest_index():
    """A head row duplicated onto another column, 37 further (another tile of the vocabulary): where it was the arg-max, two logits are the
    same number and the lower column has to be reported."""
    name, B, P, T = "TINY", 3, 6, 201
    cfg = SR.CONFIGS[name]
    c, toks, targets, prompt = gpu_inputs(name, B, P, T)
    base = run(name, B, P, T)
    b0, t0 = 1, 100
    r = int(base.pred[b0, t0])
    r2 = (r + 37) % cfg.vocab_size
    sd = dict(SR.weights(cfg))
    head = sd[f"output.{t0 % cfg.num_codebooks}.weight"].clone()
    head[r2] = head[r]
    sd[f"output.{t0 % cfg.num_codebooks}.weight"] = head
    out = LlamaDecoder(state_dict=sd, config=cfg).score(toks, targets, prompt_embs=prompt, return_stages=True)
    logits = out.stages["logits"]
    assert float(logits[b0, t0, r]) == float(logits[b0, t0, r2]) == float(logits[b0, t0].max())
    assert int(out.pred[b0, t0]) == min(r, r2)
    ties = (logits == logits.amax(dim=-1, keepdim=True)).sum(dim=-1) > 1
    assert int(ties.sum()) >= 1 and torch.equal(out.pred, SR.argmax_lowest(logits))


def test_masking_counts_and_sums():
    name, B, P, T = "TINY", 3, 6, 201
    c, toks, targets, prompt = gpu_inputs(name, B, P, T)
    full = run(name, B, P, T)
    lengths = torch.tensor([T, 57, 0])
    cut = decoder(name).score(toks, targets, prompt_embs=prompt, lengths=lengths.cuda())
    listed = decoder(name).score(toks, targets, prompt_embs=prompt, lengths=lengths.tolist())
    assert same(cut, listed)
    for out, ln in ((full, None), (cut, lengths)):
        m = SR.scored_mask(c["targets"], SR.CONFIGS[name].vocab_size, ln)
        logp, pred = out.logp.cpu(), out.pred.cpu()
        assert int((c["targets"] == IGNORE).sum()) > 0 and bool((logp[~m] == 0).all()) and bool((logp[m] < 0).all())
        assert torch.equal(out.count.cpu(), m.sum(dim=-1)) and torch.equal(out.errors.cpu(), (m & (pred != c["targets"])).sum(dim=-1))
        want = torch.where(m, logp.double(), torch.zeros((), dtype=torch.float64)).sum(dim=-1)
        tol = m.sum(dim=-1) * 2.0 ** -52 * logp.double().abs().sum(dim=-1)
        assert bool(((out.sum_logp.cpu() - want).abs() <= tol).all())
        assert torch.equal(pred, full.pred.cpu())                          # the arg-max is computed for every position
    assert torch.equal(cut.logp[0], full.logp[0]) and int(cut.count[2]) == 0 and float(cut.sum_logp[2]) == 0.0
    assert float(full.nll) == pytest.approx(-float(full.sum_logp.sum()) / int(full.count.sum())) and float(full.ter) == int(full.errors.sum()) / int(full.count.sum())


def test_repeats_graph_subsets_and_chunks_are_bit_identical():
    name, B, P, T = "TINY_HD128", 3, 6, 131
    _, toks, targets, prompt = gpu_inputs(name, B, P, T)
    dec, a = decoder(name), run(name, B, P, T)
    assert same(a, dec.score(toks, targets, prompt_embs=prompt))                                   # a repeat
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = dec.score(toks, targets, prompt_embs=prompt)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert same(a, captured)                                                                       # a captured graph = plain launches
    assert same(a, dec.score(toks[1:3], targets[1:3], prompt_embs=prompt[1:3]), slice(1, 3))       # a clip does not depend on its batch
    one = dec.score(toks, targets, prompt_embs=prompt, return_stages=True, _chunk_clips=1)         # one clip per pass = unchunked
    assert same(a, one) and all(torch.equal(a.stages[k], one.stages[k]) for k in a.stages)


def test_embed_is_unchanged_without_input_dim_and_folded_with_it():
    cfg = SR.CONFIGS["TINY"]
    toks = SR.case("TINY", 3, 6, 201, stages=True)["toks"]
    k = torch.arange(toks.shape[1]) % cfg.num_codebooks
    assert torch.equal(decoder("TINY").embed(toks.cuda()).cpu(), SR.weights(cfg)["tok_embeddings.weight"][toks + k * cfg.vocab_size])
    dec = decoder("TINY_IN")
    assert torch.equal(dec.embed(toks.cuda()).cpu(), dec._weights["tok_embeddings.weight"][toks + k * cfg.vocab_size])
