"""The codebook search on its own, through the C ABI (ac_quantize / ac_quantize_ws / ac_dequantize(_ws)), against the oracle's
fp64 nearest-code answer (tests/codebook_cases.py) on codebooks designed to break it: trained-like (k-means on EnCodec features),
bit-identical and one-ulp duplicates, an all-zero code, code norms spread over 16 - 24 octaves, and dead-code outliers.

Two kinds of checks:
  * the parity policy (parity_record.tokens: exact outside fp64 near-ties of TAU relative margin, bad == 0);
  * exact checks the policy cannot make: a planted winner is returned at every position of every launch form, and a code that
    has a bit-identical lower twin is NEVER returned (exact ties go to the first index, as torch's max does), margin or not.

EnCodec's search (core.hip rvq_encode_fwd) has four launch forms, chosen by the frame count F = B * N alone (C = 1024, H = 128):
    F >= 32768            rvq_encode16_kernel<8, 3>         48 frames per wave, tile t's pick beside tile t + 1's MFMAs
    4096 < F < 32768      rvq_encode16_kernel<8, 1>         16 frames per wave
    F <= 4096             rvq_encode16_kernel<8, 1, .., 4>  4 waves share each 16-frame group, every 4th tile each (WS = 4)
    (AC_RVQ=fp32 / "rvq_exact": rvq_encode_kernel, exact fp32 products, at every F)
WavTokenizer's single 4096 x 512 table runs rvq_encode16_kernel<32, 1, false, true> (K1), Mimi rvq_encode16_kernel<16, 1, true>
(Euclidean distance), DAC dac_vq_encode_kernel (cosine on L2-normalised factorised codes)."""
import numpy as np
import pytest
import torch

import codebook_cases as cc
import parity_record
from test_oracle_golden import TAU

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_ENOMEM = -1, -3

# frame counts at every launch-form boundary; (B, N) splits of each (only F = B * N reaches the search)
F_FORMS = {
    1: "WS=4", 15: "WS=4", 16: "WS=4", 17: "WS=4", 47: "WS=4", 48: "WS=4", 49: "WS=4", 4095: "WS=4", 4096: "WS=4",
    4097: "MS=1", 32767: "MS=1",
    32768: "MS=3", 32769: "MS=3",
}
K_LIST = (1, 2, 7, 8)


def splits(F):
    out = [(1, F)]
    for d in (3, 16, 48, 64):
        if F % d == 0 and F // d > 1:
            out.append((d, F // d))
            break
    else:
        if F > 1:
            out.append((F, 1))
    return out


def _ptr(t):
    import ctypes as C

    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    import ctypes as C

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def quantize(codec, x, K, B=1, ws=False, rc_only=False):
    """ac_quantize(_ws) of frames x [F, in] (cuda fp32) split as [B, F / B] -> tokens [F, K] int64 (cpu)."""
    from audiocodecs_amd import _native

    nat = codec._native_for(x)
    F = x.shape[0]
    N = F // B
    x = x.contiguous()
    toks = torch.full((F, max(K, 1)), -7, dtype=torch.int64, device=x.device)
    with torch.cuda.device(nat.device):
        if ws:
            w = torch.empty(max(1, nat.lib.ac_quantizer_workspace_bytes(nat.h, B, N)), dtype=torch.uint8, device=x.device)
            rc = nat.lib.ac_quantize_ws(nat.h, _ptr(x), B, N, K, _ptr(toks), _ptr(w), w.numel(), _stream())
        else:
            rc = nat.lib.ac_quantize(nat.h, _ptr(x), B, N, K, _ptr(toks), _stream())
        if rc_only:
            return rc
        _native.check(rc, nat.h, "ac_quantize")
    torch.cuda.synchronize()
    return toks.cpu()


def check_tokens(codec_name, case, toks, gold, margin, canon, C, exact_rows=None, exact_want=None):
    """The policy (bad == 0, recorded for the PARITY line), every token in range, no code with a lower bit-identical twin, and
    exact equality on `exact_rows`."""
    t = toks.numpy()
    assert t.min() >= 0 and t.max() < C, (t.min(), t.max())
    _, bad, _ = parity_record.tokens(codec_name, case, t[None], gold.numpy()[None], margin.numpy()[None], TAU)
    if bad:
        safe = np.cumprod(margin.numpy() > TAU, axis=-1).astype(bool)
        f, k = np.nonzero((t != gold.numpy()) & safe)
        detail = [(int(a), int(b), int(t[a, b]), int(gold[a, b]), float(margin[a, b])) for a, b in zip(f[:8], k[:8])]
        raise AssertionError(f"{case}: {bad} tokens differ outside fp64 near-ties (frame, stage, got, fp64, margin): {detail}")
    K = t.shape[1]
    for k in range(K):
        twin = canon[k][toks[:, k]] != toks[:, k]
        assert not bool(twin.any()), f"{case}: stage {k} returned the higher of two identical codes at frames {twin.nonzero()[:8].flatten().tolist()}"
    if exact_rows is not None:
        got = toks[exact_rows][:, :K]
        want = exact_want[:, :K]
        assert torch.equal(got, want), f"{case}: planted / tie frames {(got != want).any(1).nonzero()[:8].flatten().tolist()} wrong"


# ----------------------------------------------------------------------------------------------- EnCodec handles
@pytest.fixture(scope="module")
def enc_base(checkpoints):
    cfg, sd = checkpoints("full", 0)
    return cfg, sd


@pytest.fixture(scope="module")
def encodec_with(enc_base):
    """(name, E) -> an EnCodec wrapper whose first E.shape[0] codebooks are E (finalize packs them: split16 image, norms); cached
    for the module and released at its end."""
    import gc

    from audiocodecs_amd import Encodec

    cache = {}

    def get(name, E):
        if name not in cache:
            cfg, sd = enc_base
            sd = dict(sd)
            for q in range(E.shape[0]):
                p = f"quantizer.layers.{q}.codebook"
                sd[f"{p}.embed"] = E[q].clone()
                sd[f"{p}.embed_avg"] = E[q].clone()
            cache[name] = Encodec(24000, num_codebooks=8, state_dict=sd).eval()
        return cache[name]

    yield get
    torch.cuda.synchronize()
    cache.clear()
    gc.collect()


class Pool:
    """Query rows with their fp64 answer: frames of every case are gathered from these rows, so the oracle runs once."""

    def __init__(self, E, rows, exact_idx, exact_want, kind="encodec", K=8, **kw):
        self.E, self.x = E, rows
        self.gold, self.margin = cc.nearest_codes_fp64(kind, rows, K, E=E, **kw)
        self.canon = cc.canonical_codes(cc.search_tables(kind, E))
        self.exact_idx = exact_idx                # pool rows whose answer is checked exactly (all its stages)
        self.exact_want = exact_want              # [len(exact_idx), K]
        self.xd = rows.cuda()

    def frames(self, F, last=None):
        P = self.x.shape[0]
        idx = torch.arange(F) % P if F <= P else (torch.arange(F) * 37 + 11) % P
        if last is not None:
            idx[-1] = last
        return idx

    def run(self, codec, name, case, idx, K, B=1, C=1024, ws=False, exact_idx=None, exact_want=None):
        """exact_idx / exact_want: the exact rows of this call (default: the pool's)."""
        exact_idx = self.exact_idx if exact_idx is None else exact_idx
        exact_want = self.exact_want if exact_want is None else exact_want
        toks = quantize(codec, self.xd[idx.cuda()], K, B, ws)
        sel = torch.isin(idx, exact_idx)
        pos = sel.nonzero().flatten()
        want = None
        if len(pos):
            lut = torch.full((self.x.shape[0],), -1, dtype=torch.int64)
            lut[exact_idx] = torch.arange(len(exact_idx))
            want = exact_want[lut[idx[pos]]]
        check_tokens(name, case, toks, self.gold[idx][:, :K], self.margin[idx][:, :K], self.canon, C,
                     pos if len(pos) else None, want)
        return toks


@pytest.fixture(scope="module")
def designed(encodec_with):
    """Stages with duplicate pairs (same tile, adjacent tiles, tiles of different WS waves), one-ulp near-duplicates and an all-zero
    code; pool rows: planted chains, tie chains, and Gaussian frames at the codebooks' scale."""
    K, C, H = 8, 1024, 128
    E = cc.designed_stack(101, K, C, H)
    planted = cc.planted_chains(C, K, 0)
    ties = cc.tie_chains(C, K)
    rows = torch.cat([cc.planted_frames(E, planted, 0.05, 102), cc.planted_frames(E, ties, 0.05, 103),
                      torch.randn(1000, H, generator=cc.gen(104))])
    canon = cc.canonical_codes(E)
    want = torch.cat([planted, torch.stack([canon[k][ties[:, k]] for k in range(K)], 1)])
    pool = Pool(E, rows, torch.arange(len(want)), want)
    assert torch.equal(pool.gold[: len(want)], want)          # the planted / tie answers ARE the fp64 answers
    return encodec_with("designed", E), pool


def _sweep(designed, tag, Fs):
    codec, pool = designed
    last = cc.planted_codes(1024).index(1023)                  # the last frame of every F is planted on code C - 1
    for F in Fs:
        idx = pool.frames(F, last)
        for K in K_LIST:
            ref = None
            for B, N in splits(F):
                toks = pool.run(codec, "encodec", f"cbsearch{tag}_F{F}_K{K}_B{B}", idx, K, B)
                if ref is None:
                    ref = toks
                assert torch.equal(toks, ref), (F, K, B)       # only F reaches the search: every split is bit-identical


def test_launch_forms_planted_and_ties(designed):
    _sweep(designed, "", sorted(F_FORMS))


def test_launch_forms_planted_and_ties_exact_kernel(designed):
    from audiocodecs_amd import _native

    codec, pool = designed
    _native.debug_set(codec, "rvq_exact", 1)
    try:
        _sweep(designed, "_exact", [16, 17, 4096, 4097, 32769])
    finally:
        _native.debug_set(codec, "rvq_exact", 0)


def test_neighbour_independence_of_bad_frames(designed):
    codec, pool = designed
    H = pool.x.shape[1]
    for F in (64, 4000, 40000):                                # WS = 4, WS = 4, MS = 3
        idx = pool.frames(F)
        x = pool.xd[idx.cuda()].clone()
        bad = torch.tensor([3, 7, 9, 12, F - 40, F - 38, F - 33, F - 31])   # inside the first 16-frame group and one late 48-frame group
        vals = [float("nan"), float("inf"), 1e30, 0.0] * 2
        for b, v in zip(bad.tolist(), vals):
            x[b] = v if v != 1e30 else torch.full((H,), 1e30, device=x.device) * torch.sign(torch.randn(H, generator=cc.gen(b)).cuda())
        keep = torch.ones(F, dtype=torch.bool)
        keep[bad] = False
        t_bad = quantize(codec, x, 8)
        assert bool((t_bad >= 0).all() and (t_bad < 1024).all())
        t_clean = quantize(codec, x[keep.cuda()], 8)
        assert torch.equal(t_bad[keep], t_clean), F
        assert torch.equal(quantize(codec, x, 8), t_bad)


@pytest.mark.parametrize("octaves", [16, 20, 24])
def test_wide_norm_tables(encodec_with, octaves):
    """Stage 0's code norms spread geometrically over 2^0 .. 2^-octaves of the table's largest (rvq16.h packs one power-of-two
    scale per table)."""
    _norm_case(encodec_with, f"spread{octaves}", cc.with_norm_spread(cc.designed_stack(200 + octaves, 8, 1024, 128), octaves), None)


@pytest.mark.parametrize("log2f", [16, 20])
def test_outlier_code_tables(encodec_with, log2f):
    """One code of stage 0 2^16 / 2^20 above the rest: Mimi's embed_sum / clamp(cluster_usage, 1e-5) of a dead code."""
    _norm_case(encodec_with, f"outlier{log2f}", cc.with_outlier(cc.designed_stack(300 + log2f, 8, 1024, 128), 900, 2.0 ** log2f), 900)


def _norm_case(encodec_with, name, E, outlier):
    K, C, H = 8, 1024, 128
    codes = list(range(0, C, 37)) + cc.planted_codes(C)
    one = torch.tensor([[c] for c in codes])
    special = [cc.ZERO_CODE] + ([outlier] if outlier is not None else [])
    g = cc.gen(401)
    smin = float(E[0].double().norm(dim=1)[E[0].double().norm(dim=1) > 0].min())
    rows = torch.cat([
        cc.planted_frames(E, one, 0.05, 402),                                   # near codes of every scale (K = 1 answer exact)
        cc.planted_frames(E, torch.tensor([[c] for c in special]), 0.05, 403),  # the zero code; the outlier
        (torch.randn(8, H, generator=g, dtype=torch.float64) * smin * 1e-3 / H ** 0.5).float(),   # far nearer zero than any code
        torch.cat([torch.randn(40, H, generator=g) * 2.0 ** -j for j in range(0, 25, 3)]),        # Gaussian frames at every scale
    ])
    ex = torch.arange(len(codes) + len(special) + 8)
    want1 = torch.tensor(codes + special + [cc.ZERO_CODE] * 8)
    pool = Pool(E, rows, ex, want1[:, None])                # planted on stage 0 only: exact at K = 1
    assert torch.equal(pool.gold[ex, 0], want1)
    codec = encodec_with(name, E)
    no_rows = torch.empty(0, dtype=torch.int64)
    for F in (len(rows), 5000, 32768):
        idx = pool.frames(F)
        t1 = pool.run(codec, "encodec", f"cbsearch_{name}_F{F}_K1", idx, 1)
        # K = 8: the later stages are the policy's; stage 0 must still be the K = 1 answer, planted rows included
        t8 = pool.run(codec, "encodec", f"cbsearch_{name}_F{F}_K8", idx, 8, exact_idx=no_rows, exact_want=no_rows)
        assert torch.equal(t8[:, :1], t1)


# ----------------------------------------------------------------------------------------------- k-means (trained-like) tables
@pytest.fixture(scope="module")
def kmeans(enc_base, encodec_with):
    from test_split16_gpu import _speech_like_batch

    cfg, sd = enc_base
    base = encodec_with("synthetic", torch.stack([sd[f"quantizer.layers.{q}.codebook.embed"] for q in range(8)]))
    sig = _speech_like_batch()
    with torch.no_grad():
        train = torch.cat([base.sig_to_feats(torch.roll(sig, 53 * s, dims=1).cuda()).reshape(-1, cfg.hidden_size) for s in range(6)])
        held = base.sig_to_feats((sig.flip(-1) * 0.7).cuda()).reshape(-1, cfg.hidden_size)
    E = cc.kmeans_codebooks(train, 8, cfg.codebook_size, iters=10, seed=7)
    codec = encodec_with("kmeans", E)
    pool = Pool(E, held.cpu(), torch.empty(0, dtype=torch.int64), None)
    # the policy's band (fp64 margin relative to the best distance <= TAU), widened ONLY by tokens the reference formula cannot
    # resolve in fp32: a gap below FP32_TIE_ULPS ulps of |r|^2 + |e|^2 (codebook_cases.cancellation_margins); those get margin 0
    canc = cc.cancellation_margins(E, pool.x, pool.gold)
    pool.oracle_margin = pool.margin
    pool.margin = torch.where(canc <= cc.FP32_TIE_ULPS * 2.0 ** -24, torch.zeros_like(canc), pool.margin)
    return codec, pool, base, sig


def _excused(margin):
    return int((~np.cumprod(margin.numpy() > TAU, axis=-1).astype(bool)).sum())


def _kmeans_case(kmeans, tag):
    codec, pool, _, _ = kmeans
    P = pool.x.shape[0]
    # the fp32 band must stay a small addition to the policy's: most tokens of the trained tables are compared exactly
    n, by_policy, by_both = pool.gold.numel(), _excused(pool.oracle_margin), _excused(pool.margin)
    parity_record.record("encodec", f"cbsearch_kmeans{tag}_band", tokens_excused_by_policy=by_policy, tokens_excused_with_fp32_band=by_both)
    assert by_both <= 0.1 * n and by_both - by_policy <= 0.02 * n, (n, by_policy, by_both)
    toks = pool.run(codec, "encodec", f"cbsearch_kmeans{tag}_F{P}_K8", torch.arange(P), 8)
    big = pool.frames(32769)                                   # MS = 3 over the same rows, and MS = 1
    tb = pool.run(codec, "encodec", f"cbsearch_kmeans{tag}_F32769_K8", big, 8)
    assert torch.equal(tb, toks[big])
    tm = pool.run(codec, "encodec", f"cbsearch_kmeans{tag}_F5000_K8", big[:5000], 8)
    assert torch.equal(tm, toks[big[:5000]])


def test_kmeans_codebooks(kmeans):
    _kmeans_case(kmeans, "")


def test_kmeans_codebooks_exact_kernel(kmeans):
    from audiocodecs_amd import _native

    codec = kmeans[0]
    _native.debug_set(codec, "rvq_exact", 1)
    try:
        _kmeans_case(kmeans, "_exact")
    finally:
        _native.debug_set(codec, "rvq_exact", 0)


def test_isolated_entry_is_the_production_search(kmeans):
    _, _, base, sig = kmeans
    for codec in (base, kmeans[0]):
        x = sig.cuda()
        toks = codec.sig_to_toks(x)
        feats = codec.sig_to_feats(x)
        B, N, H = feats.shape
        assert torch.equal(quantize(codec, feats.reshape(-1, H), 8, B), toks.cpu().reshape(-1, 8))


# ----------------------------------------------------------------------------------------------- dequantize
def dequantize(codec, toks, B, N, K, ws=False, rc_only=False, out_width=None):
    from audiocodecs_amd import _native

    nat = codec._native_for(toks)
    out = torch.full((B, N, out_width), float("nan"), device=toks.device)
    with torch.cuda.device(nat.device):
        if ws:
            w = torch.empty(max(1, nat.lib.ac_quantizer_workspace_bytes(nat.h, B, N)), dtype=torch.uint8, device=toks.device)
            rc = nat.lib.ac_dequantize_ws(nat.h, _ptr(toks), B, N, K, _ptr(out), _ptr(w), w.numel(), _stream())
        else:
            rc = nat.lib.ac_dequantize(nat.h, _ptr(toks), B, N, K, _ptr(out), _stream())
        if rc_only:
            return rc
        _native.check(rc, nat.h, "ac_dequantize")
    torch.cuda.synchronize()
    return out.cpu()


def test_dequantize_is_the_fp64_sum(designed):
    """qfeats = sum_k E_k[tok_k] accumulated in fp32 in k order: every element within K ulps (2^-24 relative each) of
    sum_k |E_k[tok_k]|, the magnitude the fp32 partial sums can reach."""
    codec, pool = designed
    E = pool.E.double()
    for B, N, K in ((1, 1, 1), (3, 17, 8), (2, 4096, 8), (1, 33000, 2)):
        toks = torch.randint(0, 1024, (B, N, K), generator=cc.gen(B * N + K))
        toks[0, 0] = torch.tensor([cc.ZERO_CODE] * K)
        got = dequantize(codec, toks.cuda(), B, N, K, out_width=128).double()
        ref = sum(E[k][toks[..., k]] for k in range(K))
        mag = sum(E[k][toks[..., k]].abs() for k in range(K))
        assert bool(((got - ref).abs() <= K * 2.0 ** -24 * mag).all()), (B, N, K, float((got - ref).abs().max()))
        assert bool((got[0, 0] == 0).all())


def test_mimi_dequantize_ws_is_the_fp64_reference(mimi_designed, mimi_checkpoints):
    """Mimi's ac_dequantize_ws: output_proj_s(E_sem[tok_0]) + output_proj_a(sum_k>=1 E_ac[tok_k]) against the oracle in fp64.  The
    projections run in split16 (fp32-grade: each product within 4 ulps once the dropped lo x lo term is counted, split16.h), so each
    element is within (Dq + K + 4) ulps of the fp64 sum of the magnitudes |W| |sum of codes| it is made of (the standard bound of an
    fp32 dot product of length Dq, plus the K-term code sum)."""
    from oracle import mimi_oracle as MO

    codec, pool = mimi_designed
    cfg, _ = mimi_checkpoints("full", 0)
    W64 = pool.W64
    Et = pool.E.double()
    for B, N, K in ((1, 1, 1), (2, 17, 8), (1, 4097, 8)):
        toks = torch.randint(0, cfg.codebook_size, (B, N, K), generator=cc.gen(900 + B * N + K))
        toks[0, 0, 0] = pool.dead                             # the 10^5 dead code of the semantic table
        got = dequantize(codec, toks.cuda(), B, N, K, ws=True, out_width=cfg.hidden_size).double()
        ref = MO.rvq_decode(cfg, W64, toks.permute(0, 2, 1)).permute(0, 2, 1)
        mag = 0
        for part, lo, hi in (("semantic", 0, 1), ("acoustic", 1, K)):
            if hi <= lo:
                continue
            w = W64[f"quantizer.{part}_residual_vector_quantizer.output_proj.weight"][:, :, 0].abs()
            mag = mag + sum(Et[k][toks[..., k]].abs() for k in range(lo, hi)) @ w.t()
        bound = (cfg.codebook_dim + K + 4) * 2.0 ** -24 * mag
        err = (got - ref).abs()
        assert bool((err <= bound).all()), (B, N, K, float((err / bound.clamp_min(1e-300)).max()))


def test_bad_arguments_leave_the_handle_usable(designed, mimi_designed):
    codec, pool = designed
    idx = pool.frames(64)
    x = pool.xd[idx.cuda()]
    before = quantize(codec, x, 8)
    toks = before.reshape(1, 64, 8).cuda()
    nq = 32
    for K in (nq + 1, 0, -1):
        assert quantize(codec, x, K, rc_only=True) == AC_EINVAL
        assert dequantize(codec, toks, 1, 64, K, rc_only=True, out_width=128) == AC_EINVAL
    assert torch.equal(quantize(codec, x, 8), before)
    mcodec, mpool = mimi_designed
    mx = mpool.xd[: 32]
    mt = quantize(mcodec, mx, 8, ws=True)
    assert quantize(mcodec, mx, 8, rc_only=True) == AC_EINVAL                # no workspace on a Mimi handle: the _ws entry is needed
    nat = mcodec._native_for(mx)
    out = torch.empty(1, 32, 512, device="cuda")
    assert nat.lib.ac_quantize_ws(nat.h, _ptr(mx), 1, 32, 8, _ptr(mt.cuda()), None, 0, _stream()) == AC_ENOMEM
    assert nat.lib.ac_dequantize_ws(nat.h, _ptr(mt.cuda()), 1, 32, 8, _ptr(out), None, 0, _stream()) == AC_ENOMEM
    assert nat.lib.ac_dequantize(nat.h, _ptr(mt.cuda()), 1, 32, 8, _ptr(out), _stream()) == AC_EINVAL
    assert quantize(mcodec, mx, 33, ws=True, rc_only=True) == AC_EINVAL
    assert torch.equal(quantize(mcodec, mx, 8, ws=True), mt)


# ----------------------------------------------------------------------------------------------- Mimi
@pytest.fixture(scope="module")
def mimi_designed(mimi_checkpoints):
    from audiocodecs_amd import Mimi
    from oracle import mimi_oracle as MO

    cfg, sd = mimi_checkpoints("full", 0)
    K, C, D = 8, cfg.codebook_size, cfg.codebook_dim
    E = cc.designed_stack(500, K, C, D, shrink=3.0)            # (8x per stage would sink the last stages under the projection's rounding)
    dead = 1500                                               # a dead code: usage 0 -> clamp(1e-5): 10^5 above the rest
    sd = dict(sd)
    tabs = [("semantic", 0)] + [("acoustic", q) for q in range(K - 1)]
    for k, (part, q) in enumerate(tabs):
        cb = f"quantizer.{part}_residual_vector_quantizer.layers.{q}.codebook"
        usage = torch.ones(C)
        if k in (0, 1):
            usage[dead] = 0.0
        sd[f"{cb}.cluster_usage"] = usage
        sd[f"{cb}.embed_sum"] = E[k].clone()
    W64 = MO.cast_weights(sd, torch.float64)
    Et = torch.stack([W64[f"quantizer.{p}_residual_vector_quantizer.layers.{q}.codebook.embed"] for p, q in tabs]).float()
    assert float(Et[0, dead].abs().max()) > 1e4 * float(Et[0, :dead].abs().max())
    # planted: the semantic projection lands near E_0[c], the acoustic one near the chain sum_k>=1 E_k[c_k]
    P = cc.planted_codes(C)
    ch = torch.tensor([[P[(i + 3 * k) % len(P)] for k in range(K)] for i in range(len(P))])
    ties = cc.tie_chains(C, K)
    chains = torch.cat([ch, ties])
    sem = cc.planted_frames(Et[:1], chains[:, :1], 0.05, 501).double()
    aco = cc.planted_frames(Et[1:], chains[:, 1:], 0.05, 502).double()
    Mproj = torch.cat([W64["quantizer.semantic_residual_vector_quantizer.input_proj.weight"][:, :, 0],
                       W64["quantizer.acoustic_residual_vector_quantizer.input_proj.weight"][:, :, 0]])
    feats = torch.linalg.solve(Mproj, torch.cat([sem, aco], 1).t()).t().float()
    rows = torch.cat([feats, torch.randn(600, cfg.hidden_size, generator=cc.gen(503))])
    canon = cc.canonical_codes(Et)
    want = torch.stack([canon[k][chains[:, k]] for k in range(K)], 1)
    pool = Pool(Et, rows, torch.arange(len(chains)), want, kind="mimi", K=K, cfg=cfg, W=W64)
    assert torch.equal(pool.gold[: len(chains)], want)
    # frames whose semantic projection lands on the dead code (K = 1 only: at 10^5 the fp32 rounding of the projection swamps
    # every acoustic stage, in any fp32 arithmetic)
    semd = cc.planted_frames(Et[:1], torch.full((16, 1), dead), 0.05, 504).double()
    deadx = torch.linalg.solve(Mproj, torch.cat([semd, torch.zeros_like(semd)], 1).t()).t().float()
    codec = Mimi(24000, num_codebooks=K, state_dict=sd, config=cfg).eval()
    pool.dead, pool.deadx, pool.W64 = dead, deadx, W64
    return codec, pool


def test_mimi_search(mimi_designed):
    codec, pool = mimi_designed
    for F in (15, 16, 17, 4095, 4097):
        for K in (1, 8):
            pool.run(codec, "mimi", f"cbsearch_F{F}_K{K}", pool.frames(F), K, C=2048, ws=True)
    assert bool((quantize(codec, pool.deadx.cuda(), 1, ws=True) == pool.dead).all())


# ----------------------------------------------------------------------------------------------- WavTokenizer
@pytest.mark.parametrize("table", ["designed", "outlier16"])
def test_wavtok_search(wavtok_checkpoints, table):
    from audiocodecs_amd import WavTokenizer

    cfg, sd = wavtok_checkpoints("full", 0)
    C, D = cfg.codebook_size, cfg.dimension
    E = cc.designed_stack(600, 1, C, D) * 0.1
    if table == "outlier16":
        E = cc.with_outlier(E, 3333, 2.0 ** 16)
    sd = dict(sd)
    q = "feature_extractor.encodec.quantizer.vq.layers.0._codebook"
    sd[f"{q}.embed"] = E[0].clone()
    sd[f"{q}.embed_avg"] = E[0].clone()
    codes = torch.tensor([[c] for c in cc.planted_codes(C)] + [[lo] for lo, _ in cc.duplicate_pairs(C)] +
                         [[hi] for _, hi in cc.duplicate_pairs(C)] + ([[3333]] if table == "outlier16" else []))
    rows = torch.cat([cc.planted_frames(E, codes, 0.05, 601), torch.randn(500, D, generator=cc.gen(602)) * 0.1])
    canon = cc.canonical_codes(E)
    want = canon[0][codes[:, 0]][:, None]
    pool = Pool(E, rows, torch.arange(len(codes)), want, kind="wavtok", K=1)
    assert torch.equal(pool.gold[: len(codes)], want)
    codec = WavTokenizer(24000, state_dict=sd, arch=cfg).eval()
    for F in (15, 16, 17, 4095, 4096, 4097):
        pool.run(codec, "wavtok", f"cbsearch_{table}_F{F}", pool.frames(F, last=cc.planted_codes(C).index(C - 1)), 1, C=C)


# ----------------------------------------------------------------------------------------------- DAC
def test_dac_search(dac_checkpoints):
    from audiocodecs_amd import DAC
    from oracle import dac_oracle as DO

    cfg, sd = dac_checkpoints("full", 0)
    K, C, D, H = cfg.n_codebooks, cfg.codebook_size, cfg.codebook_dim, cfg.hidden_size
    E = cc.with_duplicates(cc.gaussian_stack(700, K, C, D, shrink=1.0), cc.duplicate_pairs(C))
    for lo, hi in [(30, 31), (200, 900)]:                      # antipodal codes
        E[:, hi] = -E[:, lo]
    E[:, 500] = E[:, 77] * 4.0                                 # the same direction at 4x the norm: equal after normalisation
    sd = dict(sd)
    for k in range(K):
        sd[f"quantizer.quantizers.{k}.codebook.weight"] = E[k].clone()
    W64 = DO.cast_weights(sd, torch.float64)
    # stage-0 planted: a latent whose in_proj lands on code c's direction (minimum-norm solution)
    Win, bin_ = W64["quantizer.quantizers.0.in_proj.weight"][:, :, 0], W64["quantizer.quantizers.0.in_proj.bias"]
    P = cc.planted_codes(C) + [lo for lo, _ in cc.duplicate_pairs(C)] + [hi for _, hi in cc.duplicate_pairs(C)] + [31, 900, 77, 500]
    tgt = cc.planted_frames(E[:1], torch.tensor([[c] for c in P]), 0.02, 701).double()
    lat = (torch.linalg.pinv(Win) @ (tgt - bin_).t()).t().float()
    rows = torch.cat([lat, torch.randn(500, H, generator=cc.gen(702))])
    canon = cc.canonical_codes(cc.search_tables("dac", E))   # ties of the normalised codes: 500 -> 77 as well as the duplicates
    pool = Pool(E, rows, torch.empty(0, dtype=torch.int64), None, kind="dac", K=K, cfg=cfg, W=W64)
    want0 = canon[0][torch.tensor(P)]
    assert int(want0[P.index(500)]) == 77
    assert torch.equal(pool.gold[: len(P), 0], want0)
    codec = DAC(44100, 44100, num_codebooks=K, state_dict=sd, config=cfg).eval()
    for F in (15, 16, 17, 4095, 4097):
        idx = pool.frames(F)
        for Kq in (1, K):
            toks = pool.run(codec, "dac", f"cbsearch_F{F}_K{Kq}", idx, Kq, C=C)
            sel = idx < len(P)
            assert torch.equal(toks[sel, 0], want0[idx[sel]])
