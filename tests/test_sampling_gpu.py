"""GPU tests of fused token sampling and token resampling (audiocodecs_amd.sampling, csrc/sampling.h) against the fp64
statement of tests/sampling_ref.py, token by token: every row outside the statement's margins (2^-18, derived there) equals it, a row
inside them still returns an entry of the kept set, and at most 3 % of a case's rows are inside them (tests/test_sampling_cpu.py checks
that share from the statement alone).  What needs no margin -- argmax, membership, -inf, NaN rows, the mask, the counter addressing -- is
compared exactly."""
import numpy as np
import pytest
import torch

import parity_record
import sampling_ref as S
from golden_cases import noise

pytestmark = pytest.mark.gpu


def _sample(logits, **kw):
    from audiocodecs_amd import sample_tokens

    return sample_tokens(logits, **kw)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_against_fp64(case):
    logits, kw, want = S.case_statement(case)
    got = _sample(torch.from_numpy(logits).cuda(), **kw).cpu().numpy()
    tok, draw, cut, sampled, allowed = want
    print(f"{S.case_id(case)}: {int((got != tok).sum())} of {len(tok)} rows differ, {int(S.excused(draw, cut).sum())} excused")
    share = S.compare(got, *want)
    parity_record.record("sampling", "excused_gpu/" + S.case_id(case), share=float(share), differ=int((got != tok).sum()))
    _, Cv = logits.shape
    exact = {k: v for k, v in kw.items() if k in ("top_k", "top_p")}
    if exact in ({"top_k": 1}, {"top_p": 0.0}):
        assert np.array_equal(got, logits.argmax(axis=1))      # (numpy's argmax returns the first of equal maxima)


@pytest.mark.parametrize("Cv", [64, 1024, 1025, 5000])
def test_argmax_modes_are_exact_with_ties(Cv):
    l = S.case_logits(64, Cv, 3.0, rounded=True)
    l[:, ::7] = l.max()      # the maximum many times over in every row
    l[5, :] = 0.0            # a constant row: index 0
    l[6, :] = -0.0
    l[6, 3] = 0.0            # -0 ties with +0: index 0, not 3
    dev = torch.from_numpy(l).cuda()
    want = l.argmax(axis=1)
    assert want[6] == 0 and want[5] == 0
    for mode in (dict(top_k=1), dict(top_p=0.0)):
        for temp in (0.7, 1.0, 1.3):
            assert np.array_equal(_sample(dev, temp=temp, seed=9, **mode).cpu().numpy(), want), (mode, temp)


@pytest.mark.parametrize("Cv", [17, 1024, 1025, 4096])
def test_special_rows(Cv):
    """-inf entries are never returned, a row with one finite entry returns it, rows of -inf and rows holding a NaN or +inf return -1, and
    the rows beside them are what they are without them."""
    R = 64
    l = S.case_logits(R, Cv, 3.0).copy()
    clean = l.copy()
    ninf = np.float32(-np.inf)
    l[::2, ::3] = ninf                       # every other row: a third of the entries are -inf
    l[1, :] = ninf                           # nothing
    l[3, :] = ninf
    l[3, Cv - 1] = -40.0                     # one finite entry, the last
    l[5, :] = ninf
    l[5, 0] = 1e30                           # ... the first
    l[7, Cv // 2] = np.nan
    l[9, 1] = np.inf
    l[11, :] = np.nan
    dev = torch.from_numpy(l).cuda()
    for mode in ({}, dict(top_k=min(50, Cv)), dict(top_k=Cv), dict(top_p=0.9), dict(top_p=1.0), dict(top_p=0.0)):
        got = _sample(dev, seed=4, offset=100, **mode).cpu().numpy()
        assert list(got[[1, 3, 5, 7, 9, 11]]) == [-1, Cv - 1, 0, -1, -1, -1], mode
        rest = np.setdiff1d(np.arange(R), [1, 3, 5, 7, 9, 11])
        assert (got[rest] >= 0).all() and (got[rest] < Cv).all()
        assert np.isfinite(l[rest, got[rest]]).all(), mode                          # never an index whose logit is -inf
        untouched = rest[rest % 2 == 1]
        assert np.array_equal(got[untouched], _sample(torch.from_numpy(clean).cuda(), seed=4, offset=100, **mode).cpu().numpy()[untouched]), mode
        S.compare(got, *S.sample(l, seed=4, offset=100, **mode))


@pytest.mark.parametrize("mode", [dict(top_k=5), dict(top_k=64), dict(top_p=0.3), dict(top_p=0.9)], ids=str)
@pytest.mark.parametrize("Cv", [65, 1024, 1025])
def test_every_result_lies_in_the_kept_set(Cv, mode):
    """Exact for top-k (decided on the logits' bits); for top-p on the rows whose cut is outside the margin."""
    l = S.case_logits(64, Cv, 3.0, rounded=Cv != 1024)
    dev = torch.from_numpy(l).cuda()
    for offset in (0, 1000, 2000):
        got = _sample(dev, seed=6, offset=offset, **mode).cpu().numpy()
        tok, draw, cut, sampled, allowed = S.sample(l, seed=6, offset=offset, **mode)
        for r in range(len(got)):
            if cut[r] >= S.DELTA:
                assert allowed(r)[got[r]], (r, got[r])


def test_counter_addressing():
    l = S.case_logits(64, 1000, 3.0)
    dev = torch.from_numpy(l).cuda()
    for mode in ({}, dict(top_k=50), dict(top_p=0.9)):
        whole = _sample(dev, seed=1, offset=40, **mode)
        assert torch.equal(whole, _sample(dev, seed=1, offset=40, **mode))
        assert torch.equal(whole[10:37], _sample(dev[10:37], seed=1, offset=50, **mode))
        assert not torch.equal(whole, _sample(dev, seed=2, offset=40, **mode))
        assert not torch.equal(whole, _sample(dev, seed=1, offset=41, **mode))
        assert torch.equal(whole, _sample(dev, seed=1, offset=torch.tensor([40], device="cuda"), **mode))
        assert torch.equal(whole, _sample(dev, seed=1, offset=torch.tensor(40, device="cuda"), **mode))
    big = 1 << 40      # the counter is 64 bits wide
    assert np.array_equal(_sample(dev, seed=1, offset=big).cpu().numpy(), S.sample(l, seed=1, offset=big)[0])
    lead = _sample(dev.view(4, 16, 1000), seed=1, offset=40)
    assert lead.shape == (4, 16) and torch.equal(lead.flatten(), _sample(dev, seed=1, offset=40))
    assert _sample(dev[:0], seed=1).shape == (0,)


def test_graph_replays_advance_the_stream():
    l = S.case_logits(64, 1025, 3.0)
    dev = torch.from_numpy(l).cuda()
    eager = [_sample(dev, top_p=0.9, seed=8, offset=64 * i) for i in range(3)]
    offset = torch.zeros(1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _sample(dev, top_p=0.9, seed=8, offset=offset)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = _sample(dev, top_p=0.9, seed=8, offset=offset)
    for i in range(3):
        g.replay()
        assert torch.equal(out, eager[i]), i
        offset += 64


def test_row_stride_and_row_index():
    from audiocodecs_amd import _native
    from audiocodecs_amd import prng
    from audiocodecs_amd.sampling import STREAM

    l = S.case_logits(64, 1000, 3.0)
    wide = torch.full((64, 1100), float("nan"))
    wide[:, 50:1050] = torch.from_numpy(l)
    view = wide.cuda()[:, 50:1050]
    assert view.stride() == (1100, 1) and not view.is_contiguous()
    want = _sample(torch.from_numpy(l).cuda(), top_k=50, seed=3)
    assert torch.equal(_sample(view, top_k=50, seed=3), want)
    assert torch.equal(_sample(torch.from_numpy(l).cuda().T.contiguous().T, top_k=50, seed=3), want)      # (no unit stride: copied)

    dev = torch.from_numpy(l).cuda()
    L = _native.lib()
    key = int(prng.key_for(3, STREAM))
    for index in (np.arange(63, -1, -1), np.array([5, 5, 5, 0, 63, 5, 0, 0, 17]), np.array([63])):
        idx = torch.from_numpy(index.astype(np.int64)).cuda()
        out = torch.full((len(index),), -7, dtype=torch.int64, device="cuda")
        rc = L.ac_sample_tokens(_native._ptr(dev), 1000, _native._ptr(idx), len(index), 1000, 1.0, 0, 0.9, key, 12, None, -1.0, None, _native._ptr(out),
                                _native._stream())
        assert rc == 0
        S.compare(out.cpu().numpy(), *S.sample(l, top_p=0.9, seed=3, offset=12, row_index=index))


# ---- resampling on the codecs' own tables ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codecs():
    from audiocodecs_amd import Encodec, Mimi, WavTokenizer, checkpoint
    from audiocodecs_amd.config import MIMI_TINY, TINY, WAVTOK_TINY

    made = {}

    def get(name):
        if name not in made:
            if name == "encodec_tiny":
                codec = Encodec(24000, num_codebooks=8, state_dict=checkpoint.synthetic_state_dict(TINY, seed=0), config=TINY).eval()
            elif name == "mimi_tiny":
                codec = Mimi(24000, num_codebooks=4, state_dict=checkpoint.synthetic_mimi_state_dict(MIMI_TINY, seed=0), config=MIMI_TINY).eval()
            else:
                codec = WavTokenizer(24000, state_dict=checkpoint.synthetic_wavtok_state_dict(WAVTOK_TINY, seed=0), arch=WAVTOK_TINY).eval()
            toks = codec.sig_to_toks(noise(31, 2, 4000).cuda())
            made[name] = (codec, toks, codec.logits().cpu().numpy())
        return made[name]

    return get


RESAMPLE_MODES = [dict(), dict(top_k=50, temp=1.3), dict(top_p=0.9, temp=0.1)]


@pytest.mark.parametrize("name", ["encodec_tiny", "mimi_tiny", "wavtok_tiny"])
def test_resample_against_fp64(codecs, name):
    codec, toks, table = codecs(name)
    K, Cv, _ = table.shape
    assert toks.shape[-1] == K and int(toks.max()) < Cv
    flat = toks.cpu().numpy().reshape(-1)
    index = flat + (np.arange(flat.size) % K) * Cv
    pooled = []
    for mode in RESAMPLE_MODES:
        for p, offset in ((0.2, 0), (0.5, 7), (0.5, 5000), (1.0, 0), (1.0, 10000), (1.0, 20000)):
            got = codec.resample(toks, p=p, seed=2, offset=offset, **mode)
            assert got.shape == toks.shape and got.dtype == toks.dtype and got is not toks
            got = got.cpu().numpy().reshape(-1)
            tok, draw, cut, sampled, allowed = S.sample(table.reshape(K * Cv, Cv), seed=2, offset=offset, row_index=index, mask_p=p, fallback=flat, **mode)
            assert np.array_equal(got != flat, sampled)                  # the mask, exactly: a masked token never keeps its value
            assert np.array_equal(got[~sampled], flat[~sampled])
            assert (got >= 0).all() and (got < Cv).all()
            if p == 1.0:
                assert sampled.all()
            ex = S.excused(draw, cut) & sampled
            wrong = np.flatnonzero((got != tok) & ~ex)
            assert wrong.size == 0, (mode, p, offset, wrong[:5], got[wrong[:5]], tok[wrong[:5]])
            for r in np.flatnonzero((got != tok) & ex):
                assert allowed(r)[got[r]]
            pooled.append((int(ex.sum()), int(sampled.sum())))
    share = sum(e for e, _ in pooled) / sum(n for _, n in pooled)
    parity_record.record("sampling", "excused_gpu/resample/" + name, share=share, rows=sum(n for _, n in pooled))
    assert share <= S.CAP, pooled


def test_resample_edges(codecs):
    from audiocodecs_amd import resample_tokens

    codec, toks, table = codecs("encodec_tiny")
    assert codec.resample(toks, p=0.0, seed=1) is toks and codec.resample(toks, p=-1.0, seed=1) is toks
    assert torch.equal(codec.resample(toks, p=0.3, seed=1, offset=9), resample_tokens(toks, codec.logits(), 0.3, seed=1, offset=9))
    assert torch.equal(codec.resample(toks.to(torch.int32), p=0.3, seed=1, offset=9), codec.resample(toks, p=0.3, seed=1, offset=9).to(torch.int32))
    with pytest.raises(NotImplementedError):
        codec.resample(toks, p=0.3, top_k=5, top_p=0.5, seed=1)
    # the torch path (no seed) is what it was: tests/test_gpu_parity.py's shapes and range
    r = codec.resample(toks, p=0.5)
    assert r.shape == toks.shape and int(r.max()) < 1024 and int(r.min()) >= 0
    for kw in (dict(top_k=10), dict(top_p=0.8)):
        r = codec.resample(toks, p=0.5, **kw)
        assert r.shape == toks.shape and int(r.max()) < 1024


def test_resample_allocates_no_row_matrix():
    """[8, 750, 8] tokens at C = 1024: the torch path gathers a [48000, 1024] fp32 matrix (197 MB) and softmaxes it; the fused call's peak
    stays below that matrix alone."""
    from audiocodecs_amd import prng, resample_tokens

    K, Cv = 8, 1024
    table = torch.randn(K, Cv, Cv, generator=torch.Generator().manual_seed(5)).cuda()
    toks = torch.from_numpy(prng.randint(5, "toks", [8, 750, K], Cv)).cuda()
    resample_tokens(toks, table, 0.2, seed=0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = resample_tokens(toks, table, 0.2, seed=0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert peak < toks.numel() * Cv * 4, peak
    assert peak <= 4 * toks.numel() * 8, peak      # the row index, the result, and nothing of the order of the table
    changed = (out != toks).float().mean().item()
    assert 0.18 < changed < 0.22
