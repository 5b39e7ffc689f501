"""CPU-side checks of the token statistics (audiocodecs_amd.tokstats, csrc/tokstats.h): the host statements against the recorded results
of the reference's own class, the form chooser, and every refusal that needs no GPU."""
import ctypes as C

import pytest
import torch

import tokstats_ref as R

FIXTURE = R.load_fixture()
IDS = [s[0] for s in FIXTURE]


def _lib():
    from audiocodecs_amd import _native

    return _native.lib()


@pytest.mark.parametrize("case", FIXTURE, ids=IDS)
def test_restatement_reproduces_the_recorded_summaries(case):
    """The fp32 restatement, appended clip by clip as the reference was, returns the recorded rounded figures exactly."""
    name, K, Cv, clips, recorded = case
    counts, total = R.ref32_counts(clips, K, Cv)
    assert total == sum(c.shape[1] for c in clips)
    assert R.ref32_summary(counts, total, Cv) == recorded


@pytest.mark.parametrize("case", FIXTURE, ids=IDS)
def test_fp64_statement_is_within_one_quantum_of_the_recorded_summaries(case):
    """What the GPU test asks of the device holds for the fp64 statement on the host: within 0.01, one quantum of the reference's rounding."""
    name, K, Cv, clips, recorded = case
    toks, lens, nvalid = R.padded_batch(clips)
    hist = R.histogram(toks, Cv, nvalid)
    assert torch.equal(hist, torch.stack([c.to(torch.int64) for c in R.ref32_counts(clips, K, Cv)[0]]))
    got = R.summary64(hist)
    for key, want in recorded.items():
        assert abs(got[key] - want) <= 0.01 + 1e-9, (key, got[key], want)


def test_fixture_covers_what_it_should():
    shapes = {(K, Cv) for _, K, Cv, _, _ in FIXTURE}
    assert {K for K, _ in shapes} == {1, 8, 9} and {Cv for _, Cv in shapes} == {512, 1024, 2048}
    kinds = {name.split("_")[0] for name in IDS}
    assert kinds >= {"uniform", "zipf", "onebin", "twobins"}
    for _, K, Cv, clips, _ in FIXTURE:
        for clip in clips:
            assert clip.shape[0] == 1 and clip.shape[2] == K and 0 <= int(clip.min()) and int(clip.max()) < Cv


def test_padded_batch_lens_stay_clear_of_half_integers():
    """The relative lens the GPU test passes: lens * N lies within 1e-4 of the clip's own length, far from a rounding boundary."""
    for _, _, _, clips, _ in FIXTURE:
        toks, lens, nvalid = R.padded_batch(clips)
        prod = lens.to(torch.float64) * toks.shape[1]
        assert float((prod - nvalid).abs().max()) < 1e-4
        assert torch.equal(prod.round().to(torch.int64), nvalid)


@pytest.mark.parametrize("K, Cv, form", [(8, 1024, ("tiled", 8)), (8, 2048, ("tiled", 8)), (1, 16384, ("tiled", 1)), (1, 65536, ("direct", 0)),
                                         (9, 1024, ("tiled", 9)), (3, 1000, ("tiled", 3)), (1, 4096, ("tiled", 1)), (64, 2, ("tiled", 64)),
                                         (1, 16385, ("direct", 0)), (64, 1 << 20, ("direct", 0))])
def test_form_is_a_pure_function_of_the_shape(K, Cv, form):
    from audiocodecs_amd.tokstats import tokstats_form

    assert tokstats_form(K, Cv) == form
    assert tokstats_form(K, Cv) == form      # (asked twice: no state)
    if form[0] == "tiled":
        assert form[1] * Cv * 4 <= 65536 and 1 <= form[1] <= K


def test_form_splits_the_codebooks_when_they_do_not_fit():
    from audiocodecs_amd.tokstats import tokstats_form

    kind, G = tokstats_form(32, 2048)
    assert kind == "tiled" and 1 <= G < 32 and G * 2048 * 4 <= 65536


@pytest.mark.parametrize("K, Cv", [(0, 1024), (-1, 1024), (65, 1024), (8, 1), (8, 0), (8, -5), (8, (1 << 20) + 1)])
def test_state_bytes_refuses(K, Cv):
    L = _lib()
    assert L.ac_tokstats_state_bytes(K, Cv) == 0
    assert L.ac_tokstats_form(K, Cv) == -1
    assert L.ac_tokstats_summary(None, K, Cv, None, None) == -1


def test_state_bytes_and_host_side_refusals():
    L = _lib()
    assert L.ac_tokstats_state_bytes(8, 1024) == (8 * 1024 + 2) * 8
    assert L.ac_tokstats_state_bytes(1, 2) == 4 * 8
    assert L.ac_tokstats_state_bytes(64, 1 << 20) == ((64 << 20) + 2) * 8
    fake = C.c_void_p(4096)           # never dereferenced: every call below is refused (or a no-op) on the host
    odd = C.c_void_p(4100)
    nbytes = L.ac_tokstats_state_bytes(8, 1024)
    assert L.ac_tokstats_accumulate(fake, 2, 10, 8, 1024, None, None, nbytes, None) == -1          # no state
    assert L.ac_tokstats_accumulate(fake, 2, 10, 8, 1024, None, odd, nbytes, None) == -1           # misaligned state
    assert L.ac_tokstats_accumulate(fake, 2, 10, 8, 1024, None, fake, nbytes - 8, None) == -3      # short state
    assert L.ac_tokstats_accumulate(None, 2, 10, 8, 1024, None, fake, nbytes, None) == -1          # no tokens
    assert L.ac_tokstats_accumulate(fake, -1, 10, 8, 1024, None, fake, nbytes, None) == -1
    assert L.ac_tokstats_accumulate(fake, 1 << 30, 1 << 30, 8, 1024, None, fake, nbytes, None) == -1      # B N K above 2^40
    assert L.ac_tokstats_accumulate(None, 0, 10, 8, 1024, None, fake, nbytes, None) == 0           # nothing to count: no launch
    assert L.ac_tokstats_accumulate(None, 2, 0, 8, 1024, None, fake, nbytes, None) == 0
    assert L.ac_tokstats_summary(fake, 8, 1024, None, None) == -1


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    import audiocodecs_amd as A
    from audiocodecs_amd._native import NativeError

    toks = torch.zeros(1, 4, 8, dtype=torch.int64)
    with pytest.raises(NativeError, match="no CPU fallback"):
        A.token_histogram(toks, 1024)
    with pytest.raises(NativeError, match="no CPU fallback"):
        A.codebook_stats(torch.zeros(8, 1024, dtype=torch.int64))
    with pytest.raises(NativeError, match="no CPU fallback"):
        A.TokenStatsState(8, 1024, "cpu")
    metric = A.CodebookUtil(8, 1024)
    with pytest.raises(NativeError, match="no CPU fallback"):
        metric.append(toks)
    with pytest.raises(ValueError):
        metric.append(torch.zeros(1, 4, 9, dtype=torch.int64))
    with pytest.raises(ValueError):
        A.token_histogram(toks.float(), 1024)
    with pytest.raises(ValueError):
        A.token_histogram(toks[0], 1024)
    with pytest.raises(ValueError):
        A.token_histogram(toks, 1)
    with pytest.raises(ValueError):
        A.CodebookUtil(65, 1024)
    with pytest.raises(ValueError):
        A.CodebookUtil(8, (1 << 20) + 1)
    assert metric.summarize() == {"codebook_util": 0.0, "norm_entropy": 0.0}       # nothing appended: the reference's 0 and 0
    assert metric.summarize("norm_entropy") == 0.0


def test_codec_has_the_one_pass_report():
    import inspect

    from audiocodecs_amd import Codec

    assert list(inspect.signature(Codec.resynthesis_report).parameters) == ["self", "sig", "length", "dnsmos_weights", "codebook_util"]
