"""The designed codebooks and the fp64 nearest-code answer of tests/codebook_cases.py, checked on the CPU: what the GPU codebook-search
tests rely on (deterministic generators, planted chains that ARE the fp64 answer with a wide margin, duplicates that are bit-identical
rows, and an fp64 answer that is the brute-force nearest code with the lowest index on ties)."""
import torch

import codebook_cases as cc

C, H = 1024, 128


def brute_force_rvq(E: torch.Tensor, x: torch.Tensor, K: int) -> torch.Tensor:
    """Residual search by exact pairwise distances (no matrix-product form) in fp64; ties go to the lowest index."""
    r = x.double()
    out = []
    for k in range(K):
        e = E[k].double()
        d = torch.cdist(r[None], e[None], compute_mode="donot_use_mm_for_euclid_dist")[0]
        best = d.min(dim=1, keepdim=True).values
        idx = torch.where(d == best, torch.arange(e.shape[0])[None], e.shape[0]).min(dim=1).values
        out.append(idx)
        r = r - e[idx]
    return torch.stack(out, 1)


def test_generators_are_deterministic():
    a, b = cc.designed_stack(5, 3, C, H), cc.designed_stack(5, 3, C, H)
    assert torch.equal(a, b) and not torch.equal(a, cc.designed_stack(6, 3, C, H))
    ch = cc.planted_chains(C, 3, 0)
    assert torch.equal(cc.planted_frames(a, ch, 0.1, 9), cc.planted_frames(b, ch, 0.1, 9))
    train = torch.randn(1200, 16, generator=cc.gen(1), dtype=torch.float64)
    assert torch.equal(cc.kmeans_codebooks(train, 2, 256, iters=3, seed=4), cc.kmeans_codebooks(train, 2, 256, iters=3, seed=4))
    for octaves in (16, 24):
        assert torch.equal(cc.with_norm_spread(a, octaves), cc.with_norm_spread(b, octaves))


def test_planted_chains_are_the_fp64_answer_with_a_wide_margin():
    K = 8
    E = cc.designed_stack(11, K, C, H)
    chains = torch.cat([cc.planted_chains(C, K, 0), cc.tie_chains(C, K)])
    x = cc.planted_frames(E, chains, 0.05, 12)
    toks, m = cc.nearest_codes_fp64("encodec", x, K, E=E)
    canon = cc.canonical_codes(E)
    want = torch.stack([canon[k][chains[:, k]] for k in range(K)], 1)
    assert torch.equal(toks, want)
    npl = len(cc.planted_codes(C))
    assert float(m[:npl].min()) > 1e-2                   # planted: unique winners by far
    assert bool((m[npl:] == 0).all())                    # tie chains: an exact tie at every stage, the lower index wins


def test_wide_norm_planted_codes_are_the_fp64_answer():
    for octaves in (16, 20, 24):
        E = cc.with_norm_spread(cc.designed_stack(13, 1, C, H), octaves)
        codes = torch.tensor([[c] for c in cc.planted_codes(C)])
        x = cc.planted_frames(E, codes, 0.05, 14)
        toks, m = cc.nearest_codes_fp64("encodec", x, 1, E=E)
        assert torch.equal(toks, codes) and float(m.min()) > 1e-2, octaves


def test_duplicates_are_bit_identical_rows():
    E = cc.designed_stack(3, 4, C, H)
    canon = cc.canonical_codes(E)
    for lo, hi in cc.duplicate_pairs(C):
        assert torch.equal(E[:, lo], E[:, hi]) and bool((E[:, lo] != 0).any())
        assert bool((canon[:, hi] == lo).all()) and bool((canon[:, lo] == lo).all())
    for lo, hi in cc.near_duplicate_pairs(C):
        d = (E[:, lo] != E[:, hi]).sum(1)
        assert bool((d == 1).all())
        assert bool((canon[:, hi] == hi).all())          # one ulp apart: distinct codes
    assert bool((E[:, cc.ZERO_CODE] == 0).all())
    # the duplicate pairs cover the tile relations the 4-wave shared search must merge
    rel = {(hi // 16 - lo // 16) % 4 for lo, hi in cc.duplicate_pairs(C) if hi // 16 != lo // 16}
    assert rel == {1, 2, 3} and any(lo // 16 == hi // 16 for lo, hi in cc.duplicate_pairs(C))
    assert not set(sum(cc.duplicate_pairs(C), ())) & (set(cc.planted_codes(C)) | {cc.ZERO_CODE})


def test_nearest_codes_fp64_is_the_brute_force_nearest_code():
    K = 4
    E = cc.designed_stack(21, K, C, H)
    g = cc.gen(22)
    chains = torch.cat([cc.tie_chains(C, K), cc.planted_chains(C, K, 0)])
    x = torch.cat([cc.planted_frames(E, chains, 0.3, 23), torch.randn(200, H, generator=g), E[0, [5, 9, 3, cc.ZERO_CODE]]])
    toks, m = cc.nearest_codes_fp64("encodec", x, K, E=E)
    bf = brute_force_rvq(E, x, K)
    safe = torch.cumprod((m > 1e-9).long(), 1).bool()    # past a non-exact near tie the two forms may part ways legitimately
    tie = m == 0
    assert torch.equal(toks[safe | tie], bf[safe | tie])
    assert int(tie.sum()) >= 14 * K                       # the tie chains: exact ties, lowest index in both
    # single table (WavTokenizer's form)
    Ew = cc.with_duplicates(cc.gaussian_stack(24, 1, 4096, 32), [(7, 4000), (100, 101)])
    xw = torch.cat([Ew[0, [4000, 101, 7]], torch.randn(100, 32, generator=g)])
    tw, mw = cc.nearest_codes_fp64("wavtok", xw, 1, E=Ew)
    assert torch.equal(tw, brute_force_rvq(Ew, xw, 1))
    assert tw[:3, 0].tolist() == [7, 100, 7]


def test_kmeans_codebooks_train_and_keep_dead_codes():
    g = cc.gen(30)
    centers = torch.randn(40, 16, generator=g, dtype=torch.float64) * 3
    train = centers[torch.randint(0, 40, (3000,), generator=g)] + 0.1 * torch.randn(3000, 16, generator=g, dtype=torch.float64)
    train[:200] = 0.0                                     # digital silence: identical frames
    E = cc.kmeans_codebooks(train, 2, 256, iters=6, seed=31)
    assert E.shape == (2, 256, 16) and E.dtype == torch.float32
    # stage 0 fits the data far better than its initial pick; stage 1 is trained on the residual and is much smaller
    r0 = train - E[0].double()[cc._assign(train, E[0].double())]
    assert float(r0.pow(2).mean()) < 0.05 * float(train.pow(2).mean())
    assert float(E[1].abs().max()) < float(E[0].abs().max())
