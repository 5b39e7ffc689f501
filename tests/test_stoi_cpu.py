"""CPU side of STOI (audiocodecs_amd.stoi): the fp64 statement of tests/stoi_ref.py pinned to what can be pinned
without pystoi (its FIR to scipy.signal.resample_poly, the band edges, the frame counts, the identity and the 1e-5 path), the library's
fp64 source against the statement's tables, the class bookkeeping, and every refusal that needs no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import stoi_ref as R

FRAME_PAIRS = ((6552, 30), (6553, 31), (6759, 32), (6964, 33), (7168, 34), (10240, 49), (10445, 50), (16000, 77))


def test_fir_equals_scipy_resample_poly():
    ss = pytest.importorskip("scipy.signal")
    h = R.fir()
    assert h.shape == (581,) and abs(h.sum() - 5.0) < 1e-12
    rng = np.random.default_rng(0)
    for L in (7001, 6552, 640):
        x = rng.standard_normal(L)
        want = ss.resample_poly(x, 5, 8, window=h / h.sum())
        got = R.resample10k(x)
        assert got.shape == want.shape == (-(-5 * L // 8),)
        assert np.abs(got - want).max() <= 1e-12


def test_band_edges():
    assert R.band_edges() == R.EDGES
    assert R.EDGES[0][0] == 7 and R.EDGES[-1][1] == 219
    assert all(a[1] == b[0] for a, b in zip(R.EDGES, R.EDGES[1:]))


def test_window_is_hanning_258_without_its_endpoints():
    w = R.window()
    assert w.shape == (256,) and w.min() > 0 and np.allclose(w, w[::-1], rtol=0, atol=1e-15)
    assert abs((w[:128] + w[128:]).max() - 1.0) > 1e-3          # the halves do not sum to 1: the overlap-add is no gather


def test_frame_counts():
    from audiocodecs_amd import _native, metrics

    L = _native.lib()
    for n, F in FRAME_PAIRS:
        x10 = R.resample10k(np.zeros(n))
        assert R.num_frames(n) == F == metrics.stoi_num_frames(n) == L.ac_stoi_num_frames(n) == R.frame_energies(x10).shape[0]
    assert L.ac_stoi_num_frames(408) == 0 and L.ac_stoi_num_frames(409) == 1 and L.ac_stoi_num_frames((1 << 24) + 1) == 0
    assert L.ac_stoi_workspace_bytes(3, 2, 16000) > 4 * 2 * 10000 * 4
    for P, B, n in ((0, 1, 16000), (5, 1, 16000), (1, 0, 16000), (1, 1, 408), (1, 1, (1 << 24) + 1)):
        assert L.ac_stoi_workspace_bytes(P, B, n) == 0


def test_identical_signals_score_one():
    x = R.make_ref("steady", 16000, 2)
    assert np.abs(R.scores(x, x) - 1.0).max() <= 1e-12


def test_score_falls_with_the_snr():
    ref = R.make_ref("steady", 10445, 1)
    s = [R.scores(R.make_hyp(ref, 10445, p), ref)[0] for p in range(3)]
    assert 1.0 > s[0] > s[1] > s[2] > 0.0


def test_thirty_frames_give_the_warning_value_and_thirty_one_one_segment():
    ref = R.make_ref("steady", 6552, 1)
    d = R.details(R.make_hyp(ref, 6552, 0)[0], ref[0])
    assert d["K"] == 30 and d["S"] == 0 and d["score"] == 1e-5
    ref = R.make_ref("steady", 6553, 1)
    d = R.details(R.make_hyp(ref, 6553, 0)[0], ref[0])
    assert d["K"] == 31 and d["S"] == 1 and d["segments"].shape == (1,) and d["score"] == d["segments"][0]


def test_score_is_not_symmetric():
    ref = R.make_ref("gaps", 12000, 1)
    hyp = R.make_hyp(ref, 12000, 2)
    assert abs(R.scores(hyp, ref)[0] - R.scores(ref, hyp)[0]) > 1e-3


def test_all_zero_reference_scores_zero():
    hyp = R.make_ref("steady", 8000, 1)
    assert R.scores(hyp, np.zeros_like(hyp))[0] == 0.0


def test_library_source_is_the_statements_window_basis_and_fir():
    from audiocodecs_amd import _native

    L = _native.lib()
    n = L.ac_stoi_source_count()
    assert n == 256 + 512 + 581
    src = np.zeros(n)
    assert L.ac_stoi_source(C.c_void_p(src.ctypes.data), n) == 0
    np.testing.assert_allclose(src[:256], R.window(), rtol=0, atol=1e-15)
    cos = src[256:768]
    np.testing.assert_allclose(cos, np.cos(2 * np.pi * np.arange(512) / 512), rtol=0, atol=1e-15)
    assert cos[0] == 1.0 and cos[128] == 0.0 and cos[256] == -1.0 and cos[384] == 0.0
    # the statement's basis is the window times these cosines: w[n] cos(2 pi ((k n) mod 512) / 512), the sine a quarter turn behind
    bs = R.dft_basis()
    nn, kk = np.arange(256)[:, None], np.arange(257)[None]
    np.testing.assert_allclose(src[:256, None] * cos[(nn * kk) % 512], bs[:, 0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(src[:256, None] * cos[(nn * kk + 384) % 512], bs[:, 1], rtol=0, atol=1e-15)
    np.testing.assert_allclose(src[768:], R.fir(), rtol=0, atol=1e-12)
    assert L.ac_stoi_source(None, n) == -1 and L.ac_stoi_source(C.c_void_p(src.ctypes.data), n - 1) == -3


# ---- the class's bookkeeping (stoi replaced by the statement) --------------------------------------------------------------------------
def test_metric_class_keeps_ids_and_scores(monkeypatch):
    from audiocodecs_amd import STOI, metrics

    calls = []

    def oracle(hyp, ref, sample_rate, extended=False, return_details=False):
        calls.append(sample_rate)
        return torch.from_numpy(R.scores(hyp.numpy(), ref.numpy())).float()

    monkeypatch.setattr(metrics, "stoi", oracle)
    assert issubclass(STOI, metrics._DistanceStats)
    ref = R.make_ref("steady", 6964, 3)
    hyp = np.concatenate([R.make_hyp(ref[i:i + 1], 6964, i, first=i + 1) for i in range(3)])
    want = R.scores(hyp, ref)
    hyp, ref = torch.from_numpy(hyp), torch.from_numpy(ref)
    met = STOI(16000)
    assert met.ids == [] and met.scores == []
    with pytest.raises(ValueError):
        met.summarize()
    met.append(["a", "b"], hyp[:2], ref[:2], lens=torch.ones(2))
    met.append(["c"], hyp[2:], ref[2:])
    assert met.ids == ["a", "b", "c"] and isinstance(met.scores, list)
    np.testing.assert_allclose(met.scores, want, rtol=1e-6)
    summ = met.summarize()
    assert summ["min_id"] == "c" and summ["max_id"] == "a" and summ["min_score"] == met.scores[2]
    assert met.summarize("average") == pytest.approx(float(np.mean(met.scores)))
    with pytest.raises(ValueError):
        met.append(["a"], hyp[:2], ref[:2])
    with pytest.raises(ValueError):
        met.append(["a", "b"], hyp[:2], ref[:2, :600])
    met.clear()
    assert met.ids == [] and met.scores == [] and calls == [16000, 16000]


# ---- refusals without a GPU ------------------------------------------------------------------------------------------------------------
def test_argument_errors_raise_before_any_device_work():
    from audiocodecs_amd import stoi

    x = torch.zeros(2, 8000)
    with pytest.raises(ValueError):
        stoi(x, x, 16000, extended=True)
    with pytest.raises(ValueError):
        stoi(x, torch.zeros(2, 8001), 16000)                 # shape mismatch
    with pytest.raises(ValueError):
        stoi(x, torch.zeros(3, 8000), 16000)
    with pytest.raises(ValueError):
        stoi(torch.zeros(5, 2, 8000), x, 16000)              # more hypotheses than a call takes
    with pytest.raises(ValueError):
        stoi(x[0], x[0], 16000)
    with pytest.raises(ValueError):
        stoi(torch.zeros(2, 408), torch.zeros(2, 408), 16000)        # 255 samples at 10 kHz: too short for one frame
    with pytest.raises(ValueError):
        stoi(torch.zeros(2, 612), torch.zeros(2, 612), 24000)        # 408 samples at 16 kHz
    with pytest.raises(ValueError):
        stoi(torch.zeros(1, 1).expand(1, (1 << 24) + 1), torch.zeros(1, 1).expand(1, (1 << 24) + 1), 16000)      # too long
    with pytest.raises(ValueError):
        stoi(x, x, 16000.0)
    s = stoi(torch.zeros(0, 8000), torch.zeros(0, 8000), 16000)      # an empty shard: no library call
    assert s.shape == (0,) and s.dtype == torch.float32
    out = stoi(torch.zeros(3, 0, 8000), torch.zeros(0, 8000), 16000, return_details=True)
    assert [tuple(t.shape) for t in out] == [(3, 0), (0, 38), (0,), (3, 0, 8)]
    assert out[1].dtype == torch.bool and out[2].dtype == torch.int32


def test_cpu_tensors_are_refused_not_computed():
    from audiocodecs_amd import _native, stoi

    with pytest.raises(_native.NativeError):
        stoi(torch.zeros(1, 8000), torch.zeros(1, 8000), 16000)


def test_abi_refusals_on_the_host():
    """Every refusal is decided before a launch: these calls return their codes on a machine without a GPU."""
    from audiocodecs_amd import _native

    L = _native.lib()
    a = 4096            # stand-ins for device pointers: never dereferenced on the host
    nws = L.ac_stoi_workspace_bytes(1, 1, 16000)
    args = lambda **kw: [kw.get("hyp", a), kw.get("ref", a), kw.get("P", 1), kw.get("B", 1), kw.get("L", 16000), kw.get("tab", a), kw.get("out", a), None, kw.get("nseg", None),
                         kw.get("segs", None), kw.get("ws", a), kw.get("nws", nws), None]
    for kw in (dict(hyp=None), dict(ref=None), dict(tab=None), dict(out=None), dict(ws=None), dict(hyp=a + 2), dict(ref=a + 1), dict(tab=a + 4), dict(ws=a + 8),
               dict(out=a + 2), dict(nseg=a + 2), dict(segs=a + 1), dict(L=408), dict(L=0), dict(L=(1 << 24) + 1), dict(P=5), dict(P=0), dict(B=0)):
        assert L.ac_stoi(*args(**kw)) == -1, kw
    assert L.ac_stoi(*args(nws=nws - 1)) == -3
    assert L.ac_stoi_tables(None, a, L.ac_stoi_tables_bytes(), None) == -1
    assert L.ac_stoi_tables(a, a + 8, L.ac_stoi_tables_bytes(), None) == -1
    assert L.ac_stoi_tables(a, a, L.ac_stoi_tables_bytes() - 1, None) == -3
