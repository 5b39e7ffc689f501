"""`TokenProbe` on the GPU (audiocodecs_amd.probe) against tests/token_probe_ref.py.  The bound of a tensor is
K_BOUND = 8 times the error of the fp32 statement against the fp64 statement on the same inputs, computed here (token_probe_ref.case),
never from the library's output -- the rule of tests/test_llama_gpu.py.  Shapes (token_probe_ref.CASES) are the smallest that cross the
seams: 3 clips of 37 frames with lengths 37, 20, 1 (a ragged clip tile, full length, one frame); 35 clips of 19 frames with mixed lengths
(past the 16-clip sub-tile and the 32-clip workgroup tile, two clips of length 0); the recipe width H = 512 at 2 x 75 with both poolings."""
import pytest
import torch

import token_probe_ref as PR
from audiocodecs_amd import _native

pytestmark = pytest.mark.gpu

_PROBES, _RUNS = {}, {}


def probe(cname):
    from audiocodecs_amd import TokenProbe

    if cname not in _PROBES:
        _PROBES[cname] = TokenProbe(state_dict=PR.weights(PR.CONFIGS[cname]), config=PR.CONFIGS[cname])
    return _PROBES[cname]


def gpu_inputs(name):
    c = PR.case(name)
    return c, c["inp"].cuda(), torch.tensor(c["lengths"], dtype=torch.int64).cuda()


def run(name):
    """One `forward(..., return_stages=True)` per case."""
    if name not in _RUNS:
        c, inp, lengths = gpu_inputs(name)
        _RUNS[name] = probe(PR.CASES[name][0]).forward(inp, lengths, return_stages=True)
    return _RUNS[name]


def check(what, got, s64, s32):
    bound = PR.K_BOUND * PR.err(s32, s64)
    e = PR.err(got.cpu(), s64)
    print(f"  {what}: error {e:.3g}, bound {bound:.3g}")
    assert tuple(got.shape) == tuple(s64.shape), what
    assert bound > 0.0 and e <= bound, (what, e, bound)
    return bound


def same(a, b, rows=slice(None)):
    fields = [f for f in ("frame_pred", "hyp_toks", "hyp_lens", "log_probs", "pred") if getattr(a, f) is not None]
    ok = all(torch.equal(getattr(a, f)[rows], getattr(b, f)) for f in fields)
    if a.stages is not None and b.stages is not None:
        ok = ok and all(torch.equal(a.stages[k][:, rows] if k == "layer_out" else a.stages[k][rows], b.stages[k]) for k in a.stages)
    return ok


def test_forward_exists_and_returns_the_fields():
    """Fails without the feature: the class, its configuration and the result type are new."""
    import audiocodecs_amd as A

    assert A.PROBE_TINY.hidden_size == 64 and issubclass(A.TokenProbe, _native.HandleOwner)
    c, toks, lengths = gpu_inputs("tiny3")
    B, N = toks.shape[:2]
    out = probe("TINY").forward(toks, lengths)
    assert isinstance(out, A.ProbeOutput) and out.stages is None and out.log_probs is None and out.pred is None
    for f in ("frame_pred", "hyp_toks"):
        t = getattr(out, f)
        assert t.is_cuda and tuple(t.shape) == (B, N) and t.dtype == torch.int64, f
    assert tuple(out.hyp_lens.shape) == (B,) and out.hyp_lens.dtype == torch.int64
    assert out.hyps() == [out.hyp_toks[b, :int(out.hyp_lens[b])].tolist() for b in range(B)]
    utt = probe("TINY_UTT").forward(toks, lengths)
    assert tuple(utt.log_probs.shape) == (B, 7) and tuple(utt.pred.shape) == (B,) and utt.pred.dtype == torch.int64 and utt.frame_pred is None


@pytest.mark.parametrize("name", list(PR.CASES))
def test_stages_log_probs_and_predictions(name):
    c = PR.case(name)
    cfg, s64, s32 = c["cfg"], c["s64"], c["s32"]
    out = run(name)
    st = out.stages
    if cfg.pooling is not None:
        check("pooled", st["pooled"], s64["pooled"], s32["pooled"])
    else:
        assert "pooled" not in st
    for l in range(cfg.num_layers):
        check(f"layer_out[{l}]", st["layer_out"][l], s64["layer_out"][l], s32["layer_out"][l])
    check("logits", st["logits"], s64["logits"], s32["logits"])
    check("log_probs", out.log_probs, s64["log_probs"], s32["log_probs"])
    sure = PR.gap_rule(s64["logits"], s32["logits"])
    if cfg.head == "ctc":
        valid = PR.valid_rows(c)
        left = int((~sure & valid).sum())
        print(f"  {name}: {left} of {int(valid.sum())} frames inside the gap")
        assert left <= PR.CAP * int(valid.sum())
        fp = out.frame_pred.cpu()
        assert torch.equal(fp[sure & valid], s64["frame_pred"][sure & valid])
        assert torch.equal(fp, torch.where(valid, PR.argmax_lowest(st["logits"].cpu()), torch.full_like(fp, -1)))      # the arg-max of the returned logits, everywhere
        # beyond a clip's length: exactly zero, exactly -1
        assert bool((st["layer_out"].cpu()[:, ~valid] == 0).all()) and bool((out.log_probs.cpu()[~valid] == 0).all()) and bool((fp[~valid] == -1).all())
        # the collapse of the library's own frame_pred, exactly
        hyp, lens = PR.collapse(fp, cfg.blank_id)
        assert torch.equal(out.hyp_toks.cpu(), hyp) and torch.equal(out.hyp_lens.cpu(), lens)
    else:
        assert bool(sure.all()) and torch.equal(out.pred.cpu(), s64["pred"]) and torch.equal(out.pred.cpu(), PR.argmax_lowest(st["logits"].cpu()))


def test_collapse_cases_a_repeat_across_a_blank_and_an_empty_clip():
    for name in ("tiny3", "tiny35"):
        fp = run(name).frame_pred.cpu().tolist()
        assert any(r[t] > 0 and r[t - 1] == 0 and r[t - 2] == r[t] for r in fp for t in range(2, len(r))), name
    c, out = PR.case("tiny35"), run("tiny35")
    empty = [b for b, n in enumerate(c["lengths"]) if n == 0]
    assert len(empty) == 2 and all(int(out.hyp_lens[b]) == 0 and bool((out.hyp_toks[b] == -1).all()) for b in empty)
    # a clip of blanks alone decodes to nothing as well: a head whose bias lifts the blank above everything
    cfg = c["cfg"]
    sd = dict(PR.weights(cfg))
    sd["head.bias"] = sd["head.bias"].clone()
    sd["head.bias"][cfg.blank_id] = 100.0
    from audiocodecs_amd import TokenProbe

    blank = TokenProbe(state_dict=sd, config=cfg).forward(*gpu_inputs("tiny3")[1:])
    assert blank.hyp_lens.tolist() == [0, 0, 0] and bool((blank.hyp_toks == -1).all()) and int((blank.frame_pred == cfg.blank_id).sum()) == 58


def test_backward_direction_starts_at_each_clips_last_frame():
    """The layer-0 backward half at t = 0 of the short clips is the packed-sequence value, not the value of a pass over all N frames."""
    c, out = PR.case("tiny3"), run("tiny3")
    cfg, H = c["cfg"], c["cfg"].hidden_size
    bound = PR.K_BOUND * PR.err(c["s32"]["layer_out"][0], c["s64"]["layer_out"][0])
    unpacked = PR.Statement(cfg, PR.weights(cfg), torch.float64).forward(c["inp"])["layer_out"][0]
    got = out.stages["layer_out"][0].cpu()
    for b in (1, 2):
        wrong, right = PR.err(got[b, 0, H:], unpacked[b, 0, H:]), PR.err(got[b, 0, H:], c["s64"]["layer_out"][0, b, 0, H:])
        print(f"  clip {b}: {wrong:.3g} from the statement without lengths, {right:.3g} from the statement, bound {bound:.3g}")
        assert wrong > bound >= right


def test_an_id_out_of_range_sets_the_status_word_and_spares_the_other_clips():
    c, toks, lengths = gpu_inputs("tiny3")
    p = probe("TINY")
    good = run("tiny3")
    bad = toks.clone()
    bad[1, 4, 0], bad[1, 9, 1] = c["cfg"].vocab_size, -3              # (without padding_idx the id vocab_size is out of range too)
    out = p.forward(bad, lengths, return_stages=True)
    with pytest.raises(_native.NativeError, match="2 token ids"):
        p.poll()
    p.poll()                                                          # the report cleared the word
    for rows in (slice(0, 1), slice(2, 3)):
        assert torch.equal(good.frame_pred[rows], out.frame_pred[rows]) and torch.equal(good.stages["layer_out"][:, rows], out.stages["layer_out"][:, rows])
        assert torch.equal(good.stages["pooled"][rows], out.stages["pooled"][rows]) and torch.equal(good.log_probs[rows], out.log_probs[rows])
    # the zero row: frame 4 of clip 1 is the other codebook's row times its weight alone
    w = PR.weights(c["cfg"])
    want = w["embedding.weight"][c["cfg"].vocab_size + int(toks[1, 4, 1])] * w["pooling.mlp.weight"][0, 1]
    assert torch.allclose(out.stages["pooled"][1, 4].cpu(), want, rtol=0, atol=1e-6)
    assert bool(torch.isfinite(out.stages["logits"]).all())


def test_padding_id_reads_the_extra_row():
    c, out = PR.case("att3"), run("att3")
    assert c["cfg"].padding_idx and int((c["inp"] == c["cfg"].vocab_size).sum()) > 0
    probe("TINY_ATT").poll()                                          # no status word: the id vocab_size is the padding row here


def test_nan_conventions_of_the_utterance_head():
    _, toks, _ = gpu_inputs("utt3")
    out = probe("TINY_UTT").forward(toks, torch.tensor([37, 1, 0]).cuda())
    lp = out.log_probs.cpu()
    assert bool(torch.isfinite(lp[0]).all()) and bool(torch.isnan(lp[1]).all()) and bool(torch.isnan(lp[2]).all())
    assert torch.equal(out.log_probs[0], run("utt3").log_probs[0])


def test_lengths_are_clamped_and_none_means_all_frames():
    _, toks, _ = gpu_inputs("tiny3")
    p = probe("TINY")
    full = p.forward(toks)
    over = p.forward(toks, torch.tensor([99, 37, 1 << 40]).cuda())
    assert same(full, over) and bool((full.frame_pred >= 0).all())
    under = p.forward(toks, torch.tensor([-5, 0, 37]).cuda())
    assert under.hyp_lens[:2].tolist() == [0, 0] and bool((under.frame_pred[:2] == -1).all()) and torch.equal(under.frame_pred[2], full.frame_pred[2])


@pytest.mark.parametrize("name", ["tiny35", "utt3"])
def test_repeats_graph_subsets_and_chunks_are_bit_identical(name):
    _, inp, lengths = gpu_inputs(name)
    p, a = probe(PR.CASES[name][0]), run(name)
    assert same(a, p.forward(inp, lengths, return_stages=True))                                   # a repeat
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = p.forward(inp, lengths, return_stages=True)
    torch.cuda.current_stream().wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert same(a, captured)                                                                      # a captured graph = plain launches
    assert same(a, p.forward(inp[1:3], lengths[1:3], return_stages=True), slice(1, 3))            # a clip does not depend on its batch
    assert same(a, p.forward(inp, lengths, return_stages=True, _chunk_clips=1))                   # one clip per pass = unchunked


def test_codec_probe_runs_sig_to_toks_then_the_probe():
    import dataclasses

    from audiocodecs_amd import TINY, Encodec, TokenProbe
    from audiocodecs_amd.checkpoint import synthetic_state_dict

    codec = Encodec(24000, num_codebooks=2, mode="encode", state_dict=synthetic_state_dict(TINY, seed=0), config=TINY)
    cfg = dataclasses.replace(PR.TINY, vocab_size=TINY.codebook_size)
    p = TokenProbe(state_dict=PR.weights(cfg), config=cfg)
    sig = torch.from_numpy(__import__("audiocodecs_amd").prng.normal(5, "probe.sig", (2, 4000)).astype("float32")).cuda()
    length = torch.tensor([1.0, 0.5]).cuda()
    toks = codec.sig_to_toks(sig, length)
    N = toks.shape[1]
    out = codec.probe(sig, p, length)
    want = p.forward(toks, torch.tensor([N, round(0.5 * N)], dtype=torch.int64).cuda())
    assert same(want, out) and bool((out.frame_pred[1, round(0.5 * N):] == -1).all())
