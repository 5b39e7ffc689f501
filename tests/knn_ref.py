"""The project's own fp64 statement of cosine k-NN matching (normalise, dot, sort) and the checker every k-NN test goes through.

`knn_ref` is the definition the kernels are held to: cosine similarity of the fp32 inputs computed in fp64 from L2-normalised rows,
neighbours ordered by (similarity descending, index ascending), rows without a direction (zero / denormal largest magnitude, an inf or
a NaN) never matched.  tests/test_knn_cpu.py pins it, and the checker, to tests/golden/knn_golden.npz, which the reference's own
helper wrote in fp64 (tools/make_knn_golden.py).

`check_match` leaves no case out.  With s64 the fp64 cosine similarity and s_k its k-th largest over the valid rows of the set, for
every valid query row:
  * the k = min(topk, valid rows) returned indices are distinct, valid and in range, and -1 follows them;
  * every returned index has s64 >= s_k - TAU; every valid index NOT returned has s64 <= s_k + TAU;
  * consecutive returned indices are ordered up to TAU;
  * the output row equals the fp64 mean of the rows at the returned indices within (k + 1) 2^-24 x the largest magnitude among those
    rows (an fp32 sum of k values and one multiply);
  * `sim` is within (H + 2) 2^-24 of s64 (the worst case of an fp32 chain over unit vectors).
A query row that is not valid must have indices -1 and a NaN output row.  TAU = 1e-4 is the project's near-tie threshold
(tests/test_oracle_golden.py), absolute here because similarities of unit vectors are O(1).
"""
from __future__ import annotations

import numpy as np

from test_oracle_golden import TAU

F32_TINY = float(np.finfo(np.float32).tiny)


def valid_rows(x: np.ndarray) -> np.ndarray:
    """Rows that have a direction: every element finite and the largest magnitude a normal fp32 number."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        return np.isfinite(x).all(axis=-1) & (np.abs(np.where(np.isfinite(x), x, 0)).max(axis=-1) >= F32_TINY)


def unit64(x: np.ndarray) -> np.ndarray:
    """fp64 L2-normalised rows (rows that are not valid become zero rows)."""
    x = np.asarray(x, dtype=np.float64)
    ok = valid_rows(x)
    x = np.where(ok[:, None], x, 0.0)
    amax = np.abs(x).max(axis=-1, keepdims=True)
    x = x / np.where(amax > 0, amax, 1.0)                 # (exact range reduction: the squared norm can neither overflow nor underflow)
    n = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    return x / np.where(n > 0, n, 1.0)


def cosine64(q: np.ndarray, t: np.ndarray) -> np.ndarray:
    return unit64(q) @ unit64(t).T


def knn_ref(q: np.ndarray, t: np.ndarray, topk: int):
    """-> (idx [Q, k] nearest first, sim [Q, k], neighbours [Q, k, H], mean [Q, H]) in fp64, k = min(topk, valid rows of t)."""
    s = cosine64(q, t)
    tv = valid_rows(t)
    s = np.where(tv[None], s, -np.inf)
    k = min(topk, int(tv.sum()))
    idx = np.argsort(-s, axis=-1, kind="stable")[:, :k]    # stable: equal similarities keep ascending index
    nb = np.asarray(t, dtype=np.float64)[idx]
    return idx, np.take_along_axis(s, idx, axis=-1), nb, nb.mean(axis=-2) if k else np.full((len(q), t.shape[1]), np.nan)


def check_match(idx, out, sim, q, t, k, tau=TAU):
    """Assert the whole contract above for one call; returns the worst |sim - s64| over the returned neighbours."""
    idx, q, t = np.asarray(idx), np.asarray(q, dtype=np.float32), np.asarray(t, dtype=np.float32)
    Q, H = q.shape
    M = t.shape[0]
    assert idx.shape == (Q, k), (idx.shape, (Q, k))
    if out is not None:
        out = np.asarray(out)
        assert out.shape == (Q, H) and out.dtype == np.float32
    if sim is not None:
        sim = np.asarray(sim)
        assert sim.shape == (Q, k)
    tv, qv = valid_rows(t), valid_rows(q)
    kk = min(k, int(tv.sum()))
    s64 = cosine64(q, t)
    t64 = t.astype(np.float64)
    worst_sim = 0.0
    for i in range(Q):
        if not qv[i] or kk == 0:
            assert (idx[i] == -1).all(), f"row {i}: a row without neighbours must have indices -1, got {idx[i]}"
            if out is not None:
                assert np.isnan(out[i]).all(), f"row {i}: a row without neighbours must be NaN"
            continue
        got = idx[i, :kk]
        assert (idx[i, kk:] == -1).all(), f"row {i}: -1 must follow the {kk} neighbours, got {idx[i]}"
        assert ((got >= 0) & (got < M)).all(), f"row {i}: index out of range {got}"
        assert len(set(got.tolist())) == kk, f"row {i}: repeated index {got}"
        assert tv[got].all(), f"row {i}: an invalid row was matched {got}"
        srow = np.where(tv, s64[i], -np.inf)
        s_k = np.partition(srow, M - kk)[M - kk]
        sg = srow[got]
        assert (sg >= s_k - tau).all(), f"row {i}: returned {got} with s64 {sg} below the k-th largest {s_k} - {tau}"
        rest = np.ones(M, dtype=bool)
        rest[got] = False
        rest &= tv
        if rest.any():
            assert srow[rest].max() <= s_k + tau, f"row {i}: index {int(np.argmax(np.where(rest, srow, -np.inf)))} with s64 {srow[rest].max()} above the k-th largest {s_k} + {tau} was not returned"
        assert (sg[:-1] >= sg[1:] - tau).all(), f"row {i}: neighbours out of order {got} {sg}"
        if out is not None:
            rows = t64[got]
            bound = (kk + 1) * 2.0 ** -24 * np.abs(rows).max()
            err = np.abs(out[i].astype(np.float64) - rows.mean(axis=0)).max()
            assert err <= bound, f"row {i}: output {err:.3e} from the mean of rows {got} (bound {bound:.3e})"
        if sim is not None:
            e = float(np.abs(sim[i, :kk].astype(np.float64) - sg).max())
            worst_sim = max(worst_sim, e)
            assert e <= (H + 2) * 2.0 ** -24, f"row {i}: similarity off by {e:.3e} (bound {(H + 2) * 2.0 ** -24:.3e})"
            assert np.isnan(sim[i, kk:]).all()
    return worst_sim


# ---- data for the tests (seeded, small) --------------------------------------------------------------------------------------
def gaussian(rng, n, H):
    return rng.standard_normal((n, H)).astype(np.float32)


def norm_spread(rng, n, H):
    """Gaussian rows whose norms spread over 2^-8 .. 2^8."""
    return (rng.standard_normal((n, H)) * 2.0 ** rng.uniform(-8, 8, size=(n, 1))).astype(np.float32)


def clustered(rng, n, H, centres):
    """Rows around 20 shared centres + 0.05 noise: most rows are near-ties of each other."""
    return (centres[rng.integers(0, len(centres), size=n)] + 0.05 * rng.standard_normal((n, H))).astype(np.float32)


def make_data(kind, seed, Q, M, H):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return gaussian(rng, Q, H), gaussian(rng, M, H)
    if kind == "spread":
        return norm_spread(rng, Q, H), norm_spread(rng, M, H)
    centres = rng.standard_normal((20, H))
    return clustered(rng, Q, H, centres), clustered(rng, M, H, centres)
