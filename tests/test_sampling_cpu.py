"""CPU side of fused token sampling (audiocodecs_amd.sampling, csrc/sampling.h): the fp64 statement of
tests/sampling_ref.py pinned to the PRNG and to the exact probabilities, the host-side refusals of the library and of the wrappers, and
the share of rows the statement's margins excuse on every case the GPU tests run (the cap is checked here first, without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sampling_ref as S
from audiocodecs_amd import prng


def test_reference_words_are_the_prng_streams():
    key = prng.key_for(11, "sample")
    mask, draw = S.words(11, 0, 1000)
    assert np.array_equal(mask, prng._draw(key, 1000, 0, 2)) and np.array_equal(draw, prng._draw(key, 1000, 1, 2))
    mask7, draw7 = S.words(11, 7, 100)      # an offset addresses the same stream
    assert np.array_equal(mask7, mask[7:107]) and np.array_equal(draw7, draw[7:107])
    u_mask, u = S.uniforms(11, 0, 1000)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and 0.0 <= u.min() and u.max() < 1.0
    assert np.array_equal(u, (draw >> np.uint64(40)).astype(np.float64) / 2.0 ** 24)


def test_reference_counts_follow_the_exact_probabilities():
    """Chi-square of 2^18 draws of one row of 64 logits against softmax in fp64.  The bound is the 1 - 1e-6 quantile of chi-square with 63
    degrees of freedom by Wilson-Hilferty, 63 (1 - 2 / 567 + 4.75 sqrt(2 / 567))^3 = 131.7: the draws are fixed, so this either holds or
    the statement is wrong."""
    n = 1 << 18
    logits = S.case_logits(1, 64, 1.0)
    tok = S.sample(logits, seed=2, row_index=np.zeros(n, dtype=np.int64))[0]
    prob = np.exp(logits[0].astype(np.float64) - logits[0].max())
    prob /= prob.sum()
    assert n * prob.min() > 5.0
    counts = np.bincount(tok, minlength=64)
    chi2 = float(((counts - n * prob) ** 2 / (n * prob)).sum())
    assert chi2 < 131.7, chi2


def test_reference_cuts():
    """The kept set on a row small enough to state by hand: weights 4 : 2 : 2 : 1 : 1 (temp = 1 / ln 2 on logits 2, 1, 1, 0, 0)."""
    l = np.array([[1.0, 0.0, 2.0, 1.0, 0.0]], dtype=np.float32)
    n = 4096
    idx = np.zeros(n, dtype=np.int64)
    kw = dict(temp=1.0 / np.log(2.0), seed=0, row_index=idx)
    assert set(S.sample(l, **kw)[0]) == {0, 1, 2, 3, 4}
    assert set(S.sample(l, top_k=1, **kw)[0]) == {2} and set(S.sample(l, top_p=0.0, **kw)[0]) == {2}
    assert set(S.sample(l, top_k=2, **kw)[0]) == {2, 0}                      # the tie at 1.0 goes to the lower index
    assert set(S.sample(l, top_k=4, **kw)[0]) == {2, 0, 3, 1}
    assert set(S.sample(l, top_p=0.45, **kw)[0]) == {2, 0}                   # mass before: 0, .4, .6, .8, .9
    assert set(S.sample(l, top_p=0.7, **kw)[0]) == {2, 0, 3}
    assert set(S.sample(l, top_p=1.0, **kw)[0]) == {0, 1, 2, 3, 4}
    tok, draw, cut, sampled, _ = S.sample(l, seed=0, row_index=idx, mask_p=0.25, fallback=np.full(n, 9))
    assert 0.2 < sampled.mean() < 0.3 and set(tok[~sampled]) == {9} and 9 not in tok[sampled]
    inf = np.float32(-np.inf)
    odd = np.array([[inf, inf, inf], [inf, 3.0, inf], [np.nan, 1.0, 2.0], [np.inf, 1.0, 2.0]], dtype=np.float32)
    assert list(S.sample(odd, seed=4)[0]) == [-1, 1, -1, -1]


def test_form_changes_once():
    from audiocodecs_amd import _native
    from audiocodecs_amd.sampling import sample_form

    L = _native.lib()
    forms = [L.ac_sample_form(c) for c in range(2, 16385)]
    assert set(forms) == {1, 2}
    assert sum(a != b for a, b in zip(forms, forms[1:])) == 1 and forms[0] == 1 and forms[-1] == 2
    assert L.ac_sample_form(1) == -1 and L.ac_sample_form(16385) == -1 and L.ac_sample_form(0) == -1 and L.ac_sample_form(-5) == -1
    assert sample_form(1024) == 1 and sample_form(1025) == 2
    with pytest.raises(ValueError):
        sample_form(1)


def test_library_refusals_need_no_gpu():
    """Every refusal is decided before anything touches the device: garbage pointers, no GPU."""
    from audiocodecs_amd import _native

    L = _native.lib()
    good, odd = C.c_void_p(0x10000), C.c_void_p(0x10004)
    inf, nan = float("inf"), float("nan")

    def call(logits=good, stride=1024, index=None, R=4, Cv=1024, temp=1.0, top_k=0, top_p=-1.0, offset_dev=None, mask_p=-1.0, fallback=None, out=good):
        return L.ac_sample_tokens(logits, stride, index, R, Cv, temp, top_k, top_p, 1, 0, offset_dev, mask_p, fallback, out, None)

    assert call(R=0) == 0 and call(R=0, top_k=50) == 0 and call(R=0, top_p=0.9, mask_p=0.2, fallback=good, index=good, offset_dev=good) == 0      # valid, nothing to launch
    assert call(logits=None) == -1 and call(out=None) == -1
    assert call(logits=C.c_void_p(0x10002)) == -1 and call(out=odd) == -1
    assert call(index=odd) == -1 and call(offset_dev=odd) == -1 and call(mask_p=0.5, fallback=odd) == -1
    assert call(R=-1) == -1 and call(R=1 << 31) == -1
    assert call(Cv=1, stride=1024) == -1 and call(Cv=16385, stride=16385) == -1 and call(Cv=0) == -1
    assert call(stride=1023) == -1 and call(stride=0) == -1 and call(stride=-1024) == -1
    assert call(temp=0.0) == -1 and call(temp=-1.0) == -1 and call(temp=inf) == -1 and call(temp=nan) == -1 and call(temp=1e-45) == -1
    assert call(top_k=-1) == -1 and call(top_k=1025) == -1
    assert call(top_p=1.5) == -1 and call(top_p=nan) == -1
    assert call(top_k=50, top_p=0.9) == -1 and call(top_k=1, top_p=0.0) == -1
    assert call(mask_p=1.5) == -1 and call(mask_p=nan) == -1 and call(mask_p=0.2) == -1 and call(mask_p=0.0) == -1      # the last two: no fallback


def test_wrapper_errors():
    from audiocodecs_amd import Codec, resample_tokens, sample_tokens
    from audiocodecs_amd._native import NativeError
    import inspect

    logits = torch.zeros(3, 64)
    with pytest.raises(NativeError, match="no CPU fallback"):
        sample_tokens(logits)
    with pytest.raises(NotImplementedError):
        sample_tokens(logits, top_k=5, top_p=0.5)
    for bad in (dict(temp=0.0), dict(temp=float("inf")), dict(top_p=1.5), dict(top_p=-0.1), dict(top_k=65), dict(top_k=0), dict(top_k=2.5), dict(offset=-1),
                dict(offset=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            sample_tokens(logits, **bad)
    for shape in ((3, 1), (3, 16385)):
        with pytest.raises(ValueError):
            sample_tokens(torch.zeros(shape))
    with pytest.raises(ValueError):
        sample_tokens(logits.double())
    toks, table = torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(3, 64, 64)
    assert resample_tokens(toks, table, 0.0) is toks and resample_tokens(toks, table, -1.0) is toks
    with pytest.raises(NativeError, match="no CPU fallback"):
        resample_tokens(toks, table, 0.5)
    with pytest.raises(NotImplementedError):
        resample_tokens(toks, table, 0.5, top_k=5, top_p=0.5)
    for bad in (dict(p=1.5), dict(p=0.5, temp=0.0), dict(p=0.5, top_k=65), dict(p=0.5, top_p=1.5)):
        with pytest.raises(ValueError):
            resample_tokens(toks, table, **bad)
    with pytest.raises(ValueError):
        resample_tokens(toks, torch.zeros(2, 64, 64), 0.5)
    with pytest.raises(ValueError):
        resample_tokens(toks.float(), table, 0.5)
    assert list(inspect.signature(Codec.resample).parameters) == ["self", "toks", "p", "temp", "top_k", "top_p", "seed", "offset"]
    assert inspect.signature(Codec.resample).parameters["seed"].default is None


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_excused_share_of_the_gpu_cases(case):
    """The cap of 3 % on every case the GPU tests compare, from the statement alone."""
    import parity_record

    tok, draw, cut, sampled, _ = S.case_statement(case)[2]
    share = float(S.excused(draw, cut).mean())
    parity_record.record("sampling", "excused_cpu/" + S.case_id(case), share=share)
    assert share <= S.CAP, share
    R, Cv = case[0], case[1]
    assert tok.shape == (R,) and tok.min() >= 0 and tok.max() < Cv


def _tables():
    """The logits tables (minus pairwise distance, -inf on the diagonal) of the three synthetic checkpoints the GPU tests resample on."""
    from audiocodecs_amd import checkpoint
    from audiocodecs_amd.config import MIMI_TINY, TINY, WAVTOK_TINY
    from oracle import encodec_oracle, mimi_oracle, wavtokenizer_oracle

    embs = {
        "encodec_tiny": encodec_oracle.embs(encodec_oracle.fold_weight_norm(checkpoint.synthetic_state_dict(TINY, seed=0)), 8),
        "mimi_tiny": mimi_oracle.embs(MIMI_TINY, mimi_oracle.cast_weights(checkpoint.synthetic_mimi_state_dict(MIMI_TINY, seed=0)), 4),
        "wavtok_tiny": wavtokenizer_oracle.embs(wavtokenizer_oracle.cast_weights(checkpoint.synthetic_wavtok_state_dict(WAVTOK_TINY, seed=0))),
    }
    for name, e in embs.items():
        lg = -torch.cdist(e, e)
        lg[torch.eye(lg.shape[-1]).bool().expand(len(lg), -1, -1)] = -float("inf")
        yield name, lg.numpy()


def test_excused_share_of_the_codebook_tables():
    """The same cap on rows of the codecs' own tables, every fourth row of every codebook, in the three modes the GPU test resamples with."""
    import parity_record

    for name, table in _tables():
        K, Cv, _ = table.shape
        rows = np.arange(0, K * Cv, 4)
        for mode in ({}, {"top_k": 50}, {"top_p": 0.9}):
            tok, draw, cut, _, _ = S.sample(table.reshape(K * Cv, Cv), seed=1, row_index=rows, **mode)
            share = float(S.excused(draw, cut).mean())
            parity_record.record("sampling", f"excused_cpu/{name}/{sorted(mode.items())}", share=share)
            assert share <= S.CAP, (name, mode, share)
            assert (tok != rows % Cv).all()      # (the diagonal is -inf: a draw never returns the row's own code)
