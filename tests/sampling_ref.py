"""The fp64 statement of fused token sampling (audiocodecs_amd.sampling) in numpy on the fp32 inputs, and the cases
the CPU and the GPU tests share.

`sample(logits, ...)` returns, per row, the token, its DRAW MARGIN -- min(u - lo, hi - u) for the chosen entry's interval [lo, hi) of the
normalised prefix over the kept set -- and its CUT MARGIN -- for top_p < 1 the least |mass_before(j) / Z - p| over the ranks j >= 1,
otherwise infinity.  Rank 0 is left out because its mass before is the empty sum, 0 in every arithmetic, and 0 <= p is no rounding question
(with it every row at p = 0 would count as uncertain, and p = 0 is argmax, exact); p = 1 has no cut margin because mass_before < Z holds
for every entry without any sum, which is how the kernel treats it.  A row is EXCUSED when either margin is below DELTA = 2^-18:

    v_exp_f32 is good to about 1 ulp; the argument (l - max) / temp rounds at 2^-24 |x| and only entries with |x| < 17 weigh more than
    2^-24, so a prefix is off by about 17 * 0.69 * 2^-24 = 7e-7 relative; an fp32 tree sum over C <= 16384 adds about 14 * 2^-24 = 8e-7;
    2^-18 = 3.8e-6 is about 2.5 times the total.

An excused row must still return an entry of the kept set with a positive weight; at most CAP = 3 % of a case's rows may be excused.
"""
import numpy as np

from audiocodecs_amd import prng

DELTA = 2.0 ** -18
CAP = 0.03
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_BLOCK = 1 << 21      # elements of logits a block of rows holds at a time


def words(seed, offset, n):
    """(mask words, draw words) of rows offset .. offset + n - 1: words 2 e and 2 e + 1 of the stream key_for(seed, "sample")."""
    key = prng.key_for(seed, "sample")
    with np.errstate(over="ignore"):
        e = np.uint64(offset) + np.arange(n, dtype=np.uint64)
        return (prng._mix(key + (np.uint64(2) * e + np.uint64(1)) * _GOLDEN), prng._mix(key + (np.uint64(2) * e + np.uint64(2)) * _GOLDEN))


def uniforms(seed, offset, n):
    """(u_mask, u_draw) in fp64: (word >> 40) * 2^-24, exact in fp32 too."""
    return tuple((w >> np.uint64(40)).astype(np.float64) * 2.0 ** -24 for w in words(seed, offset, n))


def _rows(l32, temp, top_k, top_p, u):
    l = l32.astype(np.float64)
    R, C = l.shape
    bad = np.isnan(l).any(axis=1)
    m = np.where(bad, 0.0, np.where(np.isnan(l), -np.inf, l).max(axis=1))
    bad |= ~np.isfinite(m)
    m = np.where(bad, 0.0, m)
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((l - m[:, None]) / temp)
    w[bad] = 1.0
    w = np.nan_to_num(w, nan=0.0, posinf=0.0)
    kept = np.ones((R, C), dtype=bool)
    cut = np.full(R, np.inf)
    if top_k is not None or (top_p is not None and top_p < 1.0):
        order = np.lexsort((np.broadcast_to(np.arange(C), (R, C)), -np.where(bad[:, None], 0.0, l)), axis=-1)      # value descending, index ascending
        if top_k is not None:
            keep_ranked = np.broadcast_to(np.arange(C) < top_k, (R, C))
        else:
            ws = np.take_along_axis(w, order, axis=1)
            before = np.concatenate([np.zeros((R, 1)), np.cumsum(ws, axis=1)[:, :-1]], axis=1)
            share = before / ws.sum(axis=1, keepdims=True)
            keep_ranked = share <= top_p
            cut = np.abs(share[:, 1:] - top_p).min(axis=1)
        kept = np.zeros((R, C), dtype=bool)
        np.put_along_axis(kept, order, keep_ranked, axis=1)
    ws = np.where(kept, w, 0.0)
    pre = np.cumsum(ws, axis=1)
    Z = pre[:, -1]
    tok = (pre > (u * Z)[:, None]).argmax(axis=1)
    hi = pre[np.arange(R), tok] / Z
    lo = (pre[np.arange(R), tok] - ws[np.arange(R), tok]) / Z
    draw = np.minimum(u - lo, hi - u)
    tok = np.where(bad, -1, tok)
    draw[bad] = np.inf
    cut[bad] = np.inf
    return tok.astype(np.int64), draw, cut, kept & (w > 0.0)


def sample(logits, temp=1.0, top_k=None, top_p=None, seed=0, offset=0, row_index=None, mask_p=None, fallback=None):
    """logits [T, C] fp32; row r reads logits[row_index[r]] (or logits[r]).  Returns (tokens [R], draw margin [R], cut margin [R],
    sampled [R] bool -- the mask -- and `allowed`, a function r -> bool [C] of the kept entries with a positive weight of row r)."""
    logits = np.asarray(logits)
    assert logits.dtype == np.float32 and logits.ndim == 2
    index = np.arange(len(logits)) if row_index is None else np.asarray(row_index)
    R, C = len(index), logits.shape[1]
    u_mask, u = uniforms(seed, offset, R)
    sampled = np.ones(R, dtype=bool) if mask_p is None else u_mask.astype(np.float32) < np.float32(mask_p)
    tok = np.full(R, -1, dtype=np.int64) if fallback is None else np.asarray(fallback).astype(np.int64).copy()
    draw, cut = np.full(R, np.inf), np.full(R, np.inf)
    todo = np.flatnonzero(sampled)
    step = max(1, _BLOCK // C)
    for a in range(0, len(todo), step):
        rows = todo[a:a + step]
        tok[rows], draw[rows], cut[rows], _ = _rows(logits[index[rows]], temp, top_k, top_p, u[rows])

    def allowed(r):
        return _rows(logits[index[r]][None], temp, top_k, top_p, u[r:r + 1])[3][0]

    return tok, draw, cut, sampled, allowed


def excused(draw, cut):
    return (draw < DELTA) | (cut < DELTA)


def compare(got, tok, draw, cut, sampled, allowed):
    """What every comparison against the statement asserts; returns the share of excused rows."""
    got = np.asarray(got)
    ex = excused(draw, cut) & sampled
    wrong = np.flatnonzero((got != tok) & ~ex)
    assert wrong.size == 0, f"{wrong.size} rows differ outside the margins, first {wrong[:5]}: got {got[wrong[:5]]}, want {tok[wrong[:5]]}"
    for r in np.flatnonzero((got != tok) & ex):
        assert 0 <= got[r] < len(allowed(r)) and allowed(r)[got[r]], f"excused row {r} returned {got[r]}, which is not in the kept set"
    share = ex.sum() / max(1, sampled.sum())
    assert share <= CAP, f"{ex.sum()} of {sampled.sum()} rows are excused"
    return share


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
_LOGITS = {}


def case_logits(R, C, sigma, rounded=False):
    """sigma * prng.normal(1, "logits", [R, C]) as fp32 (with `rounded`: to multiples of 0.5, which ties many entries exactly)."""
    if (R, C) not in _LOGITS:
        _LOGITS[R, C] = prng.normal(1, "logits", [R, C])
    l = sigma * _LOGITS[R, C]
    return (np.round(l * 2.0) / 2.0 if rounded else l).astype(np.float32)


def _mode(name, C):
    kind, v = name[0], name[1:]
    if kind == "n":
        return {}
    if kind == "k":
        return {"top_k": C if v == "C" else int(v)}
    return {"top_p": float(v)}


# (R, C, sigma, mode, temp, rounded): mode "n" plain, "k<k>" top-k ("kC": k = C), "p<p>" top-p.  1024 | 1025 is the form switch.
CASES = [
    (4096, 2, 3.0, "n", 1.0, False), (64, 2, 3.0, "kC", 0.7, False), (64, 2, 3.0, "p0.5", 1.3, False), (64, 2, 3.0, "k1", 1.0, False),
    (3, 17, 3.0, "n", 1.0, False), (3, 17, 3.0, "k1", 0.7, False), (3, 17, 3.0, "p0.9", 1.3, False), (1, 17, 3.0, "p0", 1.0, False),
    (64, 63, 3.0, "k50", 0.7, False), (64, 63, 3.0, "p0.5", 1.0, False), (64, 63, 3.0, "n", 1.3, False),
    (4096, 64, 3.0, "k64", 1.3, False), (1, 64, 3.0, "n", 1.0, False), (64, 64, 3.0, "p1", 0.7, False),
    (4096, 65, 3.0, "n", 0.7, False), (64, 65, 3.0, "k64", 1.0, False), (64, 65, 3.0, "p0.9", 0.7, False), (64, 65, 3.0, "kC", 1.3, False),
    (64, 128, 3.0, "n", 1.0, False), (64, 128, 3.0, "p0.5", 1.0, False),
    (64, 1000, 3.0, "n", 0.7, False), (64, 1000, 3.0, "k50", 1.0, False), (64, 1000, 3.0, "p0.5", 1.3, False),
    (4096, 1024, 3.0, "n", 1.0, False), (4096, 1024, 3.0, "p0.9", 1.0, False), (4096, 1024, 3.0, "k50", 1.0, False),
    (4096, 1024, 3.0, "n", 1.0, True), (4096, 1024, 3.0, "p0.9", 1.0, True), (64, 1024, 3.0, "k50", 0.7, True), (64, 1024, 3.0, "p0.5", 1.3, True),
    (64, 1024, 3.0, "k1", 1.0, False), (64, 1024, 3.0, "p0", 1.0, False), (64, 1024, 3.0, "p1", 1.3, False), (64, 1024, 3.0, "kC", 0.7, False),
    (64, 1024, 3.0, "k64", 1.3, False),
    (64, 1025, 3.0, "n", 1.0, False), (64, 1025, 3.0, "k50", 0.7, False), (64, 1025, 3.0, "p0.9", 0.7, False), (64, 1025, 3.0, "k1", 1.0, False),
    (64, 1025, 3.0, "p0", 1.0, False), (64, 1025, 3.0, "p1", 1.3, False), (64, 1025, 3.0, "kC", 1.0, False), (3, 1025, 3.0, "p0.5", 1.0, True),
    (4096, 4096, 3.0, "n", 1.0, False), (64, 4096, 3.0, "k64", 1.3, False), (64, 4096, 3.0, "p0.5", 0.7, False), (1, 4096, 3.0, "k50", 1.0, False),
    (2048, 16384, 5.0, "n", 1.0, False), (64, 16384, 5.0, "k50", 1.0, False), (64, 16384, 5.0, "p0.9", 1.0, False), (3, 16384, 5.0, "kC", 0.7, False),
]


def case_id(case):
    R, C, sigma, mode, temp, rounded = case
    return f"{R}x{C}-{mode}-t{temp}" + ("-ties" if rounded else "")


_STATED = {}


def case_statement(case, seed=3, offset=5):
    """(logits, kwargs, the statement's result) of a case, computed once per process."""
    if case not in _STATED:
        R, C, sigma, mode, temp, rounded = case
        logits = case_logits(R, C, sigma, rounded)
        kw = dict(temp=temp, seed=seed, offset=offset, **_mode(mode, C))
        _STATED[case] = (logits, kw, sample(logits, **kw))
    return _STATED[case]
