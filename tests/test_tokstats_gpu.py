"""GPU tests of the token statistics (audiocodecs_amd.tokstats, csrc/tokstats.h).  The oracle of the histogram is `torch.bincount` on the
host (tests/tokstats_ref.py) with exact integer equality: nothing here has a tolerance except the fp64 summary (1e-10 for C <= 4096, 1e-8
above: at most 2^20 terms below 0.54 at a few ulp of fp64) and the rounded figures against the reference's recorded ones (0.01: fp32 and
fp64 sums may fall on either side of a rounding boundary; tests/test_tokstats_cpu.py checks that bound on the host statement first).

Shapes: the smallest that reach every way the kernels can go -- fewer elements than a wave (1, 1, 1, 2), counts that are no multiple of the
block, K that does not divide the block (3, 9), C that is no power of two (1000), more than one workgroup (3 x 257 x 8, 2 x 129 x 32), codebook
groups as a grid dimension (K = 32 at C = 2048: G = 8), one codebook filling a quarter of the LDS budget (C = 4096), the direct form (C = 65536)."""
import functools

import pytest
import torch

import tokstats_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 2), (1, 7, 3, 1000), (2, 33, 9, 1024), (3, 257, 8, 2048), (2, 129, 32, 2048), (1, 300, 1, 4096), (1, 300, 1, 65536)]
IDS = ["x".join(str(v) for v in s) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def uniform(B, N, K, Cv):
    """(toks int64 [B, N, K] on the host, its bincount): computed once, never written to."""
    g = torch.Generator().manual_seed(1000003 * B + 1009 * N + 31 * K + Cv)
    toks = torch.randint(0, Cv, (B, N, K), generator=g)
    return toks, R.histogram(toks, Cv)


def state_of(toks, Cv, lens=None, state=None):
    from audiocodecs_amd import TokenStatsState, token_histogram

    state = state or TokenStatsState(toks.shape[-1], Cv, "cuda")
    counts = token_histogram(toks.cuda(), Cv, lens=lens, out=state)
    assert counts.data_ptr() == state.counts.data_ptr()
    return state


def host(state):
    buf = state.buf.cpu()
    return buf[:-2].view(state.num_codebooks, state.vocab_size), int(buf[-2]), int(buf[-1])


def test_the_shapes_reach_both_forms_and_a_split():
    from audiocodecs_amd.tokstats import tokstats_form

    forms = {(K, Cv): tokstats_form(K, Cv) for _, _, K, Cv in SHAPES}
    assert forms[(32, 2048)] == ("tiled", 8) and forms[(1, 65536)] == ("direct", 0) and forms[(9, 1024)] == ("tiled", 9)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_uniform_tokens(shape):
    from audiocodecs_amd import token_histogram

    B, N, K, Cv = shape
    toks, want = uniform(*shape)
    counts, total, bad = host(state_of(toks, Cv))
    assert torch.equal(counts, want) and total == B * N and bad == 0
    fresh = token_histogram(toks.cuda(), Cv)                               # without `out`: a new [K, C]
    assert fresh.dtype == torch.int64 and tuple(fresh.shape) == (K, Cv) and torch.equal(fresh.cpu(), want)
    assert torch.equal(token_histogram(toks.to(torch.int32).cuda(), Cv).cpu(), want)          # another integer dtype is converted
    into = torch.ones(K, Cv, dtype=torch.int64, device="cuda")
    assert token_histogram(toks.cuda(), Cv, out=into) is into and torch.equal(into.cpu(), want + 1)


@pytest.mark.parametrize("which", ["first", "last"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_token_equal(shape, which):
    """One bin of every codebook receives B N: the most contended case of the LDS and of the global atomics."""
    B, N, K, Cv = shape
    c = 0 if which == "first" else Cv - 1
    counts, total, bad = host(state_of(torch.full((B, N, K), c, dtype=torch.int64), Cv))
    want = torch.zeros(K, Cv, dtype=torch.int64)
    want[:, c] = B * N
    assert torch.equal(counts, want) and total == B * N and bad == 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lens_select_the_first_frames(shape):
    """nvalid of 0, N and a middle value through relative `lens`; lens * N is at least 0.25 away from a half-integer."""
    B, N, K, Cv = shape
    toks, _ = uniform(*shape)
    toks3 = torch.cat([toks[:1]] * 3)                    # three clips whatever B is
    nvalid = torch.tensor([0, N, N // 2])
    lens = torch.tensor([0.0, 1.0, (N // 2 + 0.25) / N], dtype=torch.float32)
    prod = lens.double() * N
    assert float(((prod - prod.floor()) - 0.5).abs().min()) >= 0.25 - 1e-4 and torch.equal(prod.round().long(), nvalid)
    counts, total, bad = host(state_of(toks3, Cv, lens=lens))
    assert torch.equal(counts, R.histogram(toks3, Cv, nvalid)) and total == int(nvalid.sum()) and bad == 0
    counts, total, _ = host(state_of(toks3, Cv, lens=torch.tensor([7.0, -1.0, 1.0])))          # clamped to [0, N]
    assert torch.equal(counts, R.histogram(toks3, Cv, torch.tensor([N, 0, N]))) and total == 2 * N


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ids_out_of_range_are_tallied_and_touch_nothing(shape):
    B, N, K, Cv = shape
    toks, _ = uniform(*shape)
    toks = toks.clone()
    flat = toks.view(-1)
    g = torch.Generator().manual_seed(5)
    where = torch.randperm(flat.numel(), generator=g)[:max(1, flat.numel() // 5)]
    flat[where] = torch.tensor([Cv, -1, 1 << 40])[torch.arange(len(where)) % 3]
    ok = (toks >= 0) & (toks < Cv)
    want = torch.stack([torch.bincount(toks[..., k][ok[..., k]], minlength=Cv) for k in range(K)])
    counts, total, bad = host(state_of(toks, Cv))
    assert bad == len(where) and total == B * N and torch.equal(counts, want)
    from audiocodecs_amd import CodebookUtil

    metric = CodebookUtil(K, Cv)
    metric.append(toks.cuda())
    with pytest.raises(ValueError, match=str(len(where))):
        metric.summarize()


def test_appends_accumulate_like_one_histogram_of_the_concatenation():
    from audiocodecs_amd import TokenStatsState

    K, Cv = 9, 1024
    g = torch.Generator().manual_seed(11)
    parts = [torch.randint(0, Cv, (B, N, K), generator=g) for B, N in ((1, 5), (3, 130), (2, 64))]
    state = TokenStatsState(K, Cv, "cuda")
    for part in parts:
        state_of(part, Cv, state=state)
    counts, total, bad = host(state)
    rows = torch.cat([p.reshape(-1, K) for p in parts])
    assert torch.equal(counts, R.histogram(rows[None], Cv)) and total == rows.shape[0] == 5 + 390 + 128 and bad == 0
    state.clear()
    assert int(state.buf.abs().sum()) == 0


@pytest.mark.parametrize("Cv", [1024, 65536], ids=["tiled", "direct"])
def test_counts_carry_past_32_bits_and_stay_exact_past_2_24(Cv):
    """A bin preset to 2^32 - 1 and one to 2^24 (where the reference's fp32 counts stop being exact): one append adds exactly."""
    from audiocodecs_amd import TokenStatsState

    K, N = 2, 77
    state = TokenStatsState(K, Cv, "cuda")
    state.counts[0, 3] = (1 << 32) - 1
    state.counts[1, Cv - 1] = 1 << 24
    state.total.fill_(1 << 33)
    toks = torch.empty(1, N, K, dtype=torch.int64)
    toks[..., 0] = 3
    toks[..., 1] = Cv - 1
    state_of(toks, Cv, state=state)
    counts, total, bad = host(state)
    assert int(counts[0, 3]) == (1 << 32) - 1 + N and int(counts[1, Cv - 1]) == (1 << 24) + N
    assert int(counts.sum()) == (1 << 32) - 1 + (1 << 24) + 2 * N and total == (1 << 33) + N and bad == 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_codebook_stats_match_the_fp64_statement(shape):
    from audiocodecs_amd import codebook_stats

    B, N, K, Cv = shape
    toks, hist = uniform(*shape)
    tol = 1e-10 if Cv <= 4096 else 1e-8
    state = state_of(toks, Cv)
    got = codebook_stats(state)
    assert got.dtype == torch.float64 and tuple(got.shape) == (K, 4)
    want = R.stats64(hist)
    worst = float((got.cpu() - want).abs().max())
    print(f"codebook_stats {shape}: worst |err| {worst:.3e} (tolerance {tol:g})")
    assert worst <= tol
    assert torch.equal(codebook_stats(state.counts.clone()), got)          # from counts alone: total is a row's sum; same bits


def test_codebook_stats_on_skewed_counts_of_the_largest_vocabularies():
    """Counts set directly (no tokens): a Zipf-like row over 4096 ids and every id of 65536 in use with counts up to 2^34."""
    from audiocodecs_amd import codebook_stats

    for Cv, tol in ((4096, 1e-10), (65536, 1e-8)):
        g = torch.Generator().manual_seed(Cv)
        counts = torch.stack([(1 << 34) // torch.arange(1, Cv + 1), torch.randint(1, 1 << 20, (Cv,), generator=g)])
        counts[1, -1] += int(counts[0].sum() - counts[1].sum())            # both rows sum to the same number of frames
        assert int(counts.min()) > 0
        got = codebook_stats(counts.cuda()).cpu()
        worst = float((got - R.stats64(counts)).abs().max())
        print(f"codebook_stats skewed C={Cv}: worst |err| {worst:.3e} (tolerance {tol:g})")
        assert worst <= tol


@pytest.mark.parametrize("case", R.load_fixture(), ids=lambda c: c[0])
def test_summaries_match_the_reference_class(case):
    """The fixture's clips as ONE padded batch with relative lens against what the reference's class returned clip by clip."""
    from audiocodecs_amd import CodebookUtil

    name, K, Cv, clips, recorded = case
    toks, lens, nvalid = R.padded_batch(clips)
    metric = CodebookUtil(K, Cv)
    metric.append(toks.cuda(), lens.cuda())
    got = metric.summarize()
    print(f"{name}: got {got}, the reference recorded {recorded}")
    assert set(got) == {"codebook_util", "norm_entropy"}
    for key, want in recorded.items():
        assert abs(got[key] - want) <= 0.01 + 1e-9, (key, got[key], want)
        assert metric.summarize(key) == got[key]
    counts, total, bad = host(metric.state)
    assert torch.equal(counts, R.histogram(toks, Cv, nvalid)) and total == int(nvalid.sum())
    metric.clear()
    for clip in clips:                                                     # B == 1 and no lens: the reference's own regime
        metric.append(clip.cuda())
    assert metric.summarize() == got


def test_degenerate_states_give_zeros_and_no_nan():
    from audiocodecs_amd import CodebookUtil, TokenStatsState, codebook_stats

    empty = codebook_stats(TokenStatsState(3, 1000, "cuda")).cpu()
    assert torch.equal(empty, torch.zeros(3, 4, dtype=torch.float64))
    metric = CodebookUtil(8, 1024)
    metric.append(torch.full((2, 50, 8), 17, device="cuda"))              # one id in use per codebook
    stats = codebook_stats(metric.state).cpu()
    assert not bool(torch.isnan(stats).any())
    assert torch.equal(stats[:, 0], torch.ones(8, dtype=torch.float64)) and float(stats[:, 1:].abs().max()) == 0.0
    assert metric.summarize() == {"codebook_util": 0.0, "norm_entropy": 0.0}
    metric.append(torch.zeros(2, 0, 8, dtype=torch.int64, device="cuda"))  # N == 0: nothing happens
    metric.append(torch.zeros(2, 9, 8, dtype=torch.int64, device="cuda"), lens=torch.zeros(2))
    assert metric.summarize() == {"codebook_util": 0.0, "norm_entropy": 0.0} and int(metric.state.total) == 100
    metric.clear()
    assert int(metric.state.buf.abs().sum()) == 0 and metric.summarize() == {"codebook_util": 0.0, "norm_entropy": 0.0}


def test_append_and_summary_replay_from_a_captured_graph():
    from audiocodecs_amd import CodebookUtil, codebook_stats

    B, N, K, Cv = 3, 257, 8, 2048
    toks, hist = uniform(B, N, K, Cv)
    dtoks = toks.cuda()
    metric = CodebookUtil(K, Cv)
    metric.append(dtoks)                      # eager once: the state exists, the library is loaded
    eager = codebook_stats(metric.state)
    metric.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            metric.append(dtoks)
            stats = codebook_stats(metric.state)
    torch.cuda.current_stream().wait_stream(side)
    metric.clear()                            # (whatever the capture itself may have run)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    counts, total, bad = host(metric.state)
    assert torch.equal(counts, 2 * hist) and total == 2 * B * N and bad == 0
    assert torch.equal(stats, eager)          # twice every count and twice the total: the same probabilities, the same bits
