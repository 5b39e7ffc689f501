"""CPU side of the spectral distances (audiocodecs_amd.metrics): the fp64 statement of tests/specdist_ref.py pinned to the fixture that
torch.stft wrote (tools/make_specdist_golden.py) and to torch.stft itself, the facts of the filterbank, the analytic value of a gain,
the metric classes' bookkeeping, and every refusal that needs no GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import specdist_ref as R
from conftest import GOLDEN_DIR


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "specdist_golden.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


def test_fixture_is_small_and_covers_every_kind(fixture):
    assert {m["kind"] for m in fixture[1]["cases"]} == set(R.KINDS)
    assert {m["L"] for m in fixture[1]["cases"]} == {513, 5121, 16000}
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "specdist_golden.npz")) < 100 * 1024


def test_oracle_equals_the_fixture(fixture):
    z, meta = fixture
    for c, m in enumerate(meta["cases"]):
        hyp, ref = R.make_pair(m["kind"], m["seed"], m["B"], m["L"])
        s, ml, sf, mf = R.distances(hyp, ref)
        assert sf.shape == (m["B"], 1 + m["L"] // 320)
        for got, name in ((s, "stft"), (ml, "mel"), (sf, "stft_frames"), (mf, "mel_frames")):
            np.testing.assert_allclose(got, z[f"c{c}_{name}"], rtol=1e-9, atol=0, err_msg=f"case {c} {name}")


@pytest.mark.parametrize("L", [513, 640, 5121])
def test_oracle_magnitudes_equal_torch_stft_in_fp64(L):
    x = R.make_signal("floor", L, 2, L)
    want = torch.stft(torch.from_numpy(x.astype(np.float64)), n_fft=1024, hop_length=320, window=torch.hann_window(1024, dtype=torch.float64), return_complex=True).abs().numpy()
    got = R.magnitudes(x)
    assert got.shape == (2, 1 + L // 320, 513)
    scale = np.abs(want).max()
    np.testing.assert_allclose(got.transpose(0, 2, 1), want, rtol=1e-12, atol=1e-12 * scale)


def test_filterbank_facts():
    fb = R.filterbank()
    assert fb.shape == (513, 80)
    assert (fb[0] == 0).all() and (fb[512] == 0).all()
    assert (fb.max(axis=0) > 0).all(), "an empty filter"
    assert (fb.max(axis=0) <= 1.0).all() and (fb >= 0).all()


def test_library_source_is_the_oracles_basis_and_filterbank():
    from audiocodecs_amd import _native

    L = _native.lib()
    n = L.ac_specdist_source_count()
    assert n == 1024 + 513 * 80
    src = np.zeros(n)
    assert L.ac_specdist_source(C.c_void_p(src.ctypes.data), n) == 0
    np.testing.assert_allclose(src[:1024], np.cos(2 * np.pi * np.arange(1024) / 1024), rtol=0, atol=1e-15)     # (numpy rounds the unreduced angle: 6e-16 near 2 pi)
    assert src[0] == 1.0 and src[256] == 0.0 and src[512] == -1.0 and src[768] == 0.0
    np.testing.assert_allclose(src[1024:].reshape(513, 80), R.filterbank(), rtol=0, atol=1e-12)
    assert L.ac_specdist_source(None, n) == -1 and L.ac_specdist_source(C.c_void_p(src.ctypes.data), n - 1) == -3


def test_gain_of_two_gives_the_analytic_values():
    ref = R.make_signal("floor", 5, 2, 5121)
    s, m, sf, mf = R.distances(2.0 * ref.astype(np.float64), ref)
    np.testing.assert_allclose(s, 10 * np.log10(2.0) * np.sqrt(513), rtol=1e-9)
    np.testing.assert_allclose(m, 10 * np.log10(2.0) * np.sqrt(80), rtol=1e-9)
    np.testing.assert_allclose(sf, 10 * np.log10(2.0) * np.sqrt(513), rtol=1e-9)


def test_frame_counts():
    from audiocodecs_amd import _native, metrics

    L = _native.lib()
    for n, F in ((513, 2), (640, 3), (5119, 16), (5120, 17), (5121, 17), (10560, 34), (16000, 51)):
        assert metrics.num_frames(n) == F == L.ac_specdist_num_frames(n) == R.frames(np.zeros((1, n))).shape[1]
    assert L.ac_specdist_num_frames(512) == 0 and L.ac_specdist_num_frames((1 << 24) + 1) == 0
    assert L.ac_specdist_workspace_bytes(3, 2, 16000) == 2 * 3 * 2 * 51 * 4
    for P, B, n in ((0, 1, 16000), (5, 1, 16000), (1, 0, 16000), (1, 1, 512), (1, 1, (1 << 24) + 1)):
        assert L.ac_specdist_workspace_bytes(P, B, n) == 0


# ---- the metric classes' bookkeeping (spectral_distances replaced by the oracle) ----------------------------------------------------------
def test_metric_classes_keep_ids_and_scores(monkeypatch):
    from audiocodecs_amd import MelDistance, STFTDistance, metrics

    calls = []

    def oracle(hyp, ref, sample_rate, return_frames=False):
        calls.append(sample_rate)
        s, m, _, _ = R.distances(hyp.numpy(), ref.numpy())
        return torch.from_numpy(s).float(), torch.from_numpy(m).float()

    monkeypatch.setattr(metrics, "spectral_distances", oracle)
    hyp, ref = (torch.from_numpy(a) for a in R.make_pair("noise", 3, 3, 640))
    want = R.distances(hyp.numpy(), ref.numpy())
    for cls, which in ((STFTDistance, 0), (MelDistance, 1)):
        met = cls(16000)
        assert met.ids == [] and met.scores == []
        with pytest.raises(ValueError):
            met.summarize()
        met.append(["a", "b"], hyp[:2], ref[:2], lens=torch.ones(2))
        met.append(["c"], hyp[2:], ref[2:])
        assert met.ids == ["a", "b", "c"] and isinstance(met.scores, list) and len(met.scores) == 3
        np.testing.assert_allclose(met.scores, want[which], rtol=1e-6)
        summ = met.summarize()
        lo, hi = int(np.argmin(want[which])), int(np.argmax(want[which]))
        assert summ["min_id"] == "abc"[lo] and summ["max_id"] == "abc"[hi]
        assert summ["min_score"] == met.scores[lo] and summ["max_score"] == met.scores[hi]
        assert met.summarize("average") == pytest.approx(float(np.mean(met.scores)))
        with pytest.raises(ValueError):
            met.append(["a"], hyp[:2], ref[:2])
        with pytest.raises(ValueError):
            met.append(["a", "b"], hyp[:2], ref[:2, :600])
        met.clear()
        assert met.ids == [] and met.scores == []
    assert calls == [16000] * 4


# ---- refusals without a GPU ------------------------------------------------------------------------------------------------------------
def test_only_the_defaults_are_compiled():
    from audiocodecs_amd import MelDistance, STFTDistance

    STFTDistance(24000, n_fft=1024, hop_length=320)
    MelDistance(24000, n_mels=80, n_fft=1024, hop_length=320)
    for kw in (dict(n_fft=512), dict(hop_length=256)):
        with pytest.raises(ValueError):
            STFTDistance(24000, **kw)
        with pytest.raises(ValueError):
            MelDistance(24000, **kw)
    with pytest.raises(ValueError):
        MelDistance(24000, n_mels=64)


def test_argument_errors_raise_before_any_device_work():
    from audiocodecs_amd import spectral_distances

    x = torch.zeros(2, 4000)
    with pytest.raises(ValueError):
        spectral_distances(x, torch.zeros(2, 4001), 16000)          # shape mismatch
    with pytest.raises(ValueError):
        spectral_distances(x, torch.zeros(3, 4000), 16000)
    with pytest.raises(ValueError):
        spectral_distances(torch.zeros(5, 2, 4000), x, 16000)       # more hypotheses than a call takes
    with pytest.raises(ValueError):
        spectral_distances(x[0], x[0], 16000)
    with pytest.raises(ValueError):
        spectral_distances(torch.zeros(2, 512), torch.zeros(2, 512), 16000)       # cannot be reflect-padded
    with pytest.raises(ValueError):
        spectral_distances(torch.zeros(2, 768), torch.zeros(2, 768), 24000)       # 512 samples at 16 kHz
    with pytest.raises(ValueError):
        spectral_distances(x, x, 16000.0)
    s, m = spectral_distances(torch.zeros(0, 4000), torch.zeros(0, 4000), 16000)  # an empty shard: no library call
    assert s.shape == (0,) and m.shape == (0,)
    out = spectral_distances(torch.zeros(3, 0, 4000), torch.zeros(0, 4000), 16000, return_frames=True)
    assert [tuple(t.shape) for t in out] == [(3, 0), (3, 0), (3, 0, 13), (3, 0, 13)]


def test_cpu_tensors_are_refused_not_computed():
    from audiocodecs_amd import _native, spectral_distances

    with pytest.raises(_native.NativeError):
        spectral_distances(torch.zeros(1, 4000), torch.zeros(1, 4000), 16000)


def test_abi_refusals_on_the_host():
    """Every refusal is decided before a launch: these calls return their codes on a machine without a GPU."""
    from audiocodecs_amd import _native

    L = _native.lib()
    a = 4096            # stand-ins for device pointers: never dereferenced on the host
    args = lambda **kw: [kw.get("hyp", a), kw.get("ref", a), kw.get("P", 1), 1, kw.get("L", 16000), kw.get("tab", a), kw.get("so", a), a, None, None, kw.get("ws", a),
                         kw.get("nws", 2 * 51 * 4), None]
    for kw in (dict(hyp=None), dict(ref=None), dict(tab=None), dict(so=None), dict(ws=None), dict(hyp=a + 2), dict(tab=a + 4), dict(ws=a + 8), dict(L=512), dict(P=5), dict(P=0)):
        assert L.ac_specdist(*args(**kw)) == -1, kw
    assert L.ac_specdist(*args(nws=2 * 51 * 4 - 1)) == -3
    assert L.ac_specdist_tables(None, a, L.ac_specdist_tables_bytes(), None) == -1
    assert L.ac_specdist_tables(a, a + 8, L.ac_specdist_tables_bytes(), None) == -1
    assert L.ac_specdist_tables(a, a, L.ac_specdist_tables_bytes() - 1, None) == -3
