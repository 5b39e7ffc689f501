"""CPU side of the k-NN feature matcher: the fp64 statement and the checker of tests/knn_ref.py pinned to the fixture the reference's
own helper wrote (tools/make_knn_golden.py), the checker's own teeth, host-side argument errors, and the refusals of the new entry
points on a machine without a GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import knn_ref as R
from conftest import GOLDEN_DIR


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN_DIR, "knn_golden.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


def cases(fixture):
    z, meta = fixture
    for c, m in enumerate(meta["cases"]):
        yield m, z[f"c{c}_q"].astype(np.float32), z[f"c{c}_t"].astype(np.float32), z[f"c{c}_neighbours"].astype(np.float64), z[f"c{c}_idx"].astype(np.int64), z[f"c{c}_mean"]


def test_fixture_is_the_three_cases(fixture):
    assert [(m["Q"], m["M"], m["H"], m["topk"]) for m in fixture[1]["cases"]] == [(64, 300, 32, 4), (33, 5, 128, 8), (48, 97, 512, 1)]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "knn_golden.npz")) < 200 * 1024


def test_fp64_statement_matches_the_reference_helper(fixture):
    for m, q, t, nb, idx, mean in cases(fixture):
        ridx, _, rnb, rmean = R.knn_ref(q, t, m["topk"])
        assert ridx.shape == (m["Q"], min(m["topk"], m["M"]))
        np.testing.assert_array_equal(ridx, idx)
        np.testing.assert_array_equal(rnb, nb)
        np.testing.assert_allclose(rmean, mean, rtol=0, atol=1e-12)


def _padded(idx, sim, topk):
    Q, kk = idx.shape
    i = np.full((Q, topk), -1, dtype=np.int64)
    s = np.full((Q, topk), np.nan, dtype=np.float32)
    i[:, :kk], s[:, :kk] = idx, sim
    return i, s


def test_checker_accepts_the_reference_helper(fixture):
    for m, q, t, nb, idx, mean in cases(fixture):
        i, s = _padded(idx, np.take_along_axis(R.cosine64(q, t), idx, axis=-1), m["topk"])
        R.check_match(i, mean.astype(np.float32), s, q, t, m["topk"])


def test_checker_has_teeth(fixture):
    m, q, t, nb, idx, mean = next(cases(fixture))
    k = m["topk"]
    i, s = _padded(idx, np.take_along_axis(R.cosine64(q, t), idx, axis=-1), k)
    out = mean.astype(np.float32)
    far = int(np.argmin(R.cosine64(q, t)[0]))
    for spoil in ("wrong_index", "repeat", "order", "out", "sim", "range"):
        i2, o2, s2 = i.copy(), out.copy(), s.copy()
        if spoil == "wrong_index":
            i2[0, k - 1] = far
        elif spoil == "repeat":
            i2[0, 1] = i2[0, 0]
        elif spoil == "order":
            i2[0, [0, k - 1]] = i2[0, [k - 1, 0]]
        elif spoil == "out":
            o2[0, 3] += 1e-4 * np.abs(t).max()
        elif spoil == "sim":
            s2[0, 0] += 1e-5
        else:
            i2[0, 0] = m["M"]
        with pytest.raises((AssertionError, IndexError)):
            R.check_match(i2, o2, s2, q, t, k)


def test_checker_bad_rows():
    rng = np.random.default_rng(5)
    q, t = R.gaussian(rng, 4, 32), R.gaussian(rng, 9, 32)
    t[2] = 0
    t[5, 7] = np.nan
    q[1] = 0
    assert R.valid_rows(t).tolist() == [True, True, False, True, True, False, True, True, True]
    idx, sim, nb, mean = R.knn_ref(q, t, 8)
    assert idx.shape == (4, 7) and 2 not in idx and 5 not in idx
    i, s = _padded(idx, sim, 8)
    out = mean.astype(np.float32)
    i[1], out[1] = -1, np.nan
    R.check_match(i, out, s, q, t, 8)
    i[0, 0] = 2      # an invalid row matched
    with pytest.raises(AssertionError):
        R.check_match(i, out, s, q, t, 8)


def test_host_side_argument_errors():
    from audiocodecs_amd import KnnIndex, knn, knn_match
    from audiocodecs_amd._native import NativeError

    q, t = torch.zeros(3, 32), torch.zeros(5, 32)
    for bad in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError):
            knn_match(q, t, topk=bad)
    with pytest.raises(ValueError):
        knn_match(q, torch.zeros(0, 32))
    with pytest.raises(ValueError):
        knn_match(q, torch.zeros(5, 64))
    with pytest.raises(ValueError):
        knn_match(q, torch.zeros(5))
    with pytest.raises(ValueError):
        knn_match(torch.zeros(3, 48), torch.zeros(5, 48))       # not a multiple of 32
    with pytest.raises(ValueError):
        knn_match(torch.zeros(3, 544), torch.zeros(5, 544))     # wider than the widest compiled width
    for bad in (0, 65, -2, 1.5):
        with pytest.raises(ValueError):
            knn_match(q, t, num_splits=bad)
    with pytest.raises(ValueError):
        knn(q, t, topk=0)
    with pytest.raises(ValueError):
        KnnIndex(torch.zeros(0, 32))
    # CPU tensors: there is no CPU fallback
    with pytest.raises(NativeError):
        knn_match(q, t)
    with pytest.raises(NativeError):
        knn(q, t)
    with pytest.raises(NativeError):
        KnnIndex(t)


def test_knn_vc_refuses_multi_codebook_tokens_on_the_host():
    from audiocodecs_amd import Codec

    class Stub(Codec):
        def embs(self): ...
        def _sig_to_toks(self, sig, length): ...
        def _sig_to_feats(self, sig, length): ...
        def _sig_to_qfeats(self, sig, length): ...
        def _toks_to_sig(self, toks, length): ...

    c = Stub(24000, 24000)
    with pytest.raises(ValueError):
        c.knn_vc(torch.zeros(1, 5, 8, dtype=torch.int64), [torch.zeros(100)])
    with pytest.raises(NotImplementedError):
        c.knn_vc(torch.zeros(1, 5, 1, dtype=torch.int64), [torch.zeros(100)])


def test_entry_points_refuse_bad_arguments_without_gpu():
    from audiocodecs_amd import _native

    L = _native.lib()
    EINVAL = -1
    assert L.ac_knn_packed_bytes(0, 32) == 0 and L.ac_knn_packed_bytes(5, 48) == 0 and L.ac_knn_packed_bytes((1 << 24) + 1, 32) == 0
    assert L.ac_knn_packed_bytes(17, 64) == 32 * 64 * 4 + 32 * 4
    assert L.ac_knn_pack(None, 5, 32, None, 0, None) == EINVAL
    assert L.ac_knn_num_splits(0, 5, 32, 0) == EINVAL and L.ac_knn_num_splits(5, 0, 32, 0) == EINVAL
    assert L.ac_knn_num_splits(5, 5, 48, 0) == EINVAL and L.ac_knn_num_splits(5, 5, 32, 65) == EINVAL and L.ac_knn_num_splits(5, 5, 32, -1) == EINVAL
    assert L.ac_knn_num_splits(5, 5, 32, 7) == 7
    assert L.ac_knn_workspace_bytes(5, 5, 32, 0, 1) == 0 and L.ac_knn_workspace_bytes(5, 5, 32, 9, 1) == 0 and L.ac_knn_workspace_bytes(5, 5, 48, 4, 1) == 0
    assert L.ac_knn_workspace_bytes(5, 5, 32, 3, 2) == 5 * 2 * 4 * 8 and L.ac_knn_workspace_bytes(5, 5, 32, 5, 1) == 5 * 8 * 8
    assert L.ac_knn_match(None, 5, None, None, 5, 32, 4, 0, None, None, None, None, 0, None) == EINVAL
    fake = C.c_void_p(4096)      # never dereferenced: every refusal below is decided on the host
    assert L.ac_knn_pack(fake, 5, 48, fake, 1 << 20, None) == EINVAL
    assert L.ac_knn_pack(fake, 0, 32, fake, 1 << 20, None) == EINVAL
    assert L.ac_knn_pack(C.c_void_p(4100), 5, 32, fake, 1 << 20, None) == EINVAL      # misaligned
    assert L.ac_knn_pack(fake, 5, 32, fake, 16, None) == -3                           # AC_ENOMEM: short packed buffer
    for topk in (0, 9):
        assert L.ac_knn_match(fake, 5, fake, fake, 5, 32, topk, 0, fake, None, None, fake, 1 << 20, None) == EINVAL
    assert L.ac_knn_match(fake, 5, fake, fake, 5, 48, 4, 0, fake, None, None, fake, 1 << 20, None) == EINVAL
    assert L.ac_knn_match(fake, 0, fake, fake, 5, 32, 4, 0, fake, None, None, fake, 1 << 20, None) == EINVAL
    assert L.ac_knn_match(fake, 5, fake, fake, 5, 32, 4, 65, fake, None, None, fake, 1 << 20, None) == EINVAL
    assert L.ac_knn_match(fake, 5, fake, fake, 5, 32, 4, 1, fake, None, None, fake, 16, None) == -3


def test_auto_split_choice():
    """The automatic split count: 1 from 1024 query waves on and below 16 tiles of the set, otherwise enough slices
    for 1024 waves, at least 8 tiles each, 16 at the most.  A wave owns 32 rows (16 at H = 512)."""
    from audiocodecs_amd.knn import auto_splits

    assert auto_splits(400, 240, 512) == 1 and auto_splits(400, 241, 512) == 2          # 15 tiles / 16 tiles
    assert auto_splits(400, 2400, 512) == 16 and auto_splits(400, 24000, 512) == 16
    assert auto_splits(16, 2032, 128) == 15 and auto_splits(16, 2033, 128) == 16
    assert auto_splits(16368, 24000, 512) == 2 and auto_splits(16369, 24000, 512) == 1  # 1023 / 1024 waves of 16 rows
    assert auto_splits(32736, 256, 32) == 2 and auto_splits(32737, 256, 32) == 1        # 1023 / 1024 waves of 32 rows
    assert auto_splits(8192, 24000, 512) == 2 and auto_splits(8176, 24000, 512) == 3    # 512 / 511 waves
    assert auto_splits(25600, 24000, 512) == 1
    assert auto_splits(5, 100, 96) == auto_splits(5, 100, 128)                         # a padded width is its compiled width
