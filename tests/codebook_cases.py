"""Designed codebooks and query frames for the codebook-search tests (test_codebook_search_gpu.py), plus the fp64 nearest-code
answer taken from the oracle.  Everything is deterministic (torch.Generator seeds) and runs on the CPU except the EnCodec features
that train the k-means tables, which the GPU test produces and hands to `kmeans_codebooks`.

Shapes: codebook stacks [K, C, H] fp32, query frames [F, H] fp32, tokens [F, K] int64, margins [F, K] fp64."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import torch

# fp32 resolution of the reference's distance d = |r|^2 - 2 r.e + |e|^2: its last two additions round at the scale of
# |r|^2 + |e|^2, once each per distance, and a comparison involves two distances -- 4 ulps of that scale (see cancellation_margins)
FP32_TIE_ULPS = 4
STAGE_SHRINK = 8.0     # stage k of a designed stack is 8^-k the scale of stage 0: a planted chain is then the unique fp64 answer
ZERO_CODE = 700        # the all-zero code of the designed tables (not a planted code, not in a duplicate pair)


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(int(seed))


def planted_codes(C: int) -> List[int]:
    """Winners at the first / last code of the first, second and last 16-code tiles and of the 128-code boundaries."""
    return [0, 15, 16, 127, 128, 255, C - 17, C - 16, C - 1]


def duplicate_pairs(C: int) -> List[Tuple[int, int]]:
    """(lower, higher) code pairs made bit-identical.  Tile t = code // 16; under the 4-wave shared form (rvq16.h WS) wave t % 4
    owns tile t, so the pairs cover: the same tile (first, middle and last tile), adjacent tiles, and tiles of waves 1, 2 and 3
    apart, first tile against last tile included.  Disjoint from planted_codes(C) and ZERO_CODE."""
    assert C >= 1024 and C % 128 == 0
    return [
        (3, 9),                    # first tile
        (40, 44),                  # same tile
        (323, 341),                # tiles 20 / 21: adjacent, waves 1 apart
        (487, 519),                # tiles 30 / 32: waves 2 apart
        (801, 857),                # tiles 50 / 53: waves 3 apart
        (4, C - 6),                # first tile / last tile (waves 3 apart)
        (C - 12, C - 4),           # last tile
    ]


def near_duplicate_pairs(C: int) -> List[Tuple[int, int]]:
    """(lower, higher): the higher code differs from the lower by one fp32 ulp in one element."""
    return [(600, 601), (610, 626)]


def gaussian_stack(seed: int, K: int, C: int, H: int, scale: float = 1.0, shrink: float = STAGE_SHRINK) -> torch.Tensor:
    g = gen(seed)
    E = torch.randn(K, C, H, generator=g, dtype=torch.float64)
    E *= scale * shrink ** -torch.arange(K, dtype=torch.float64)[:, None, None]
    return E.float()


def with_duplicates(E: torch.Tensor, pairs: Sequence[Tuple[int, int]]) -> torch.Tensor:
    E = E.clone()
    for lo, hi in pairs:
        E[:, hi] = E[:, lo]
    return E


def with_near_duplicates(E: torch.Tensor, pairs: Sequence[Tuple[int, int]]) -> torch.Tensor:
    E = E.clone()
    for lo, hi in pairs:
        E[:, hi] = E[:, lo]
        E[:, hi, 5] = torch.nextafter(E[:, lo, 5], torch.tensor(float("inf")))
    return E


def with_zero_code(E: torch.Tensor, code: int = ZERO_CODE) -> torch.Tensor:
    E = E.clone()
    E[:, code] = 0.0
    return E


def with_norm_spread(E: torch.Tensor, octaves: float, stage: int = 0) -> torch.Tensor:
    """Code c of `stage` scaled by 2^(-octaves * c / (C - 1)): the norms spread geometrically from the table's largest down to
    2^-octaves of it, in code order (neighbouring tiles hold neighbouring scales)."""
    E = E.clone()
    C = E.shape[1]
    s = torch.exp2(-octaves * torch.arange(C, dtype=torch.float64) / (C - 1))
    E[stage] = (E[stage].double() * s[:, None]).float()
    return E


def with_outlier(E: torch.Tensor, code: int, factor: float, stage: int = 0) -> torch.Tensor:
    """One code `factor` times larger than the rest (a dead code of a table stored as embed_sum / clamp(usage, 1e-5))."""
    E = E.clone()
    E[stage, code] = E[stage, code] * factor
    return E


def designed_stack(seed: int, K: int, C: int, H: int, scale: float = 1.0, shrink: float = STAGE_SHRINK) -> torch.Tensor:
    """Gaussian stages (8x shrink per stage) with the duplicate pairs, the near-duplicate pairs and the zero code in every stage."""
    E = gaussian_stack(seed, K, C, H, scale, shrink)
    E = with_near_duplicates(with_duplicates(E, duplicate_pairs(C)), near_duplicate_pairs(C))
    return with_zero_code(E)


def planted_frames(E: torch.Tensor, chains: torch.Tensor, noise: float, seed: int) -> torch.Tensor:
    """chains [F, K'] code indices (K' <= K): frame f = sum_k E_k[chains[f, k]] + noise * N(0, 1) scaled by the RMS of the chain's
    LAST code (so a chain ending on a small code of a wide-norm table stays near it), accumulated in fp64 and rounded once."""
    Kc = chains.shape[1]
    E64 = E.double()
    x = torch.zeros(chains.shape[0], E.shape[2], dtype=torch.float64)
    for k in range(Kc):
        x += E64[k][chains[:, k]]
    last = E64[Kc - 1][chains[:, Kc - 1]].pow(2).mean(1, keepdim=True).sqrt()
    x += noise * last * torch.randn(x.shape, generator=gen(seed), dtype=torch.float64)
    return x.float()


def planted_chains(C: int, K: int, seed: int) -> torch.Tensor:
    """One chain per planted code: stage 0 takes the planted code, later stages cycle through the planted codes as well."""
    P = planted_codes(C)
    rows = [[P[(i + 3 * k) % len(P)] for k in range(K)] for i in range(len(P))]
    return torch.tensor(rows, dtype=torch.int64)


def tie_chains(C: int, K: int) -> torch.Tensor:
    """Chains through the duplicate pairs: every stage's winner is a bit-identical pair, once through its lower member and once
    through its higher one (the fp64 answer is the lower index either way)."""
    pairs = duplicate_pairs(C)
    rows = []
    for i in range(len(pairs)):
        for side in (0, 1):
            rows.append([pairs[(i + k) % len(pairs)][side] for k in range(K)])
    return torch.tensor(rows, dtype=torch.int64)


def canonical_codes(E: torch.Tensor) -> torch.Tensor:
    """[K, C]: for each code, the lowest index holding a bit-identical row (itself when it has no lower twin)."""
    K, C, _ = E.shape
    out = torch.arange(C).repeat(K, 1)
    for k in range(K):
        seen: Dict[bytes, int] = {}
        rows = E[k].contiguous().numpy()
        for c in range(C):
            key = rows[c].tobytes()
            out[k, c] = seen.setdefault(key, c)
    return out


def search_tables(kind: str, E: torch.Tensor) -> torch.Tensor:
    """The rows the search compares: DAC's search runs on L2-normalised codes, so a code and a power-of-two multiple of it are a
    bit-identical pair there; the other searches compare the codes themselves."""
    if kind == "dac":
        return torch.nn.functional.normalize(E.double(), dim=-1)
    return E


def kmeans_codebooks(train: torch.Tensor, K: int, C: int, iters: int = 10, seed: int = 0) -> torch.Tensor:
    """Residual VQ trained in fp64: stage k runs `iters` Lloyd iterations on the residuals the stages < k leave, from C distinct
    training rows picked at random.  A code no frame picks keeps its value (a dead code); identical training frames (digital
    silence) give bit-identical codes.  train [F, H] (any device) -> [K, C, H] fp32 on the CPU."""
    x = train.detach().to(torch.float64)
    assert x.shape[0] >= C
    g = gen(seed)
    out = []
    for _ in range(K):
        E = x[torch.randperm(x.shape[0], generator=g)[:C].to(x.device)].clone()
        for _ in range(iters):
            a = _assign(x, E)
            sums = torch.zeros_like(E).index_add_(0, a, x)
            cnt = torch.bincount(a, minlength=C).to(x.dtype)
            live = cnt > 0
            E[live] = sums[live] / cnt[live, None]
        out.append(E.float().cpu())
        x = x - E.float().double()[_assign(x, E)]     # the residual against the stored (fp32) codes
    return torch.stack(out)


def _assign(x: torch.Tensor, E: torch.Tensor) -> torch.Tensor:
    d = x.pow(2).sum(1, keepdim=True) - 2 * x @ E.t() + E.pow(2).sum(1)[None]
    return d.argmin(dim=1)


def nearest_codes_fp64(kind: str, x: torch.Tensor, K: int, *, E: torch.Tensor, cfg=None, W=None):
    """The oracle's codebook search in fp64 on frames x [F, in] -> (tokens [F, K] int64, relative margins [F, K] fp64).
    kind: "encodec" (E [K', C, H]), "wavtok" (E [1, C, D], K = 1), "mimi" / "dac" (cfg and the oracle's fp64 weight dict W, the
    input projections included: x are the quantiser's inputs; E [K', C, D] the tables the search sees).
    A code with a bit-identical lower twin is mapped to the twin: the oracle's matrix-product distances are not always bit-equal
    for identical rows (a BLAS may treat the last columns of a block differently), and identical rows leave identical residuals,
    so the mapping is the first-index rule made exact without changing any later stage.  (DAC: twins of the NORMALISED codes,
    search_tables; their raw rows and so the later residuals may differ, but such a tie has margin 0, which excuses the frame's
    later stages under the policy.)"""
    z = x.to(torch.float64).t()[None]                              # [1, in, F]
    with torch.no_grad():
        if kind == "encodec":
            from oracle import encodec_oracle as O

            codes, m = O.rvq_encode([e.double() for e in E[:K]], z, True)   # [K, 1, F]
            toks, m = codes[:, 0].t(), m[:, 0].t()
        elif kind == "wavtok":
            from oracle import wavtokenizer_oracle as O

            assert K == 1
            toks, m = O.vq_encode(E[0].double(), z, True)                 # [1, F]
            toks, m = toks.t(), m.t()
        elif kind == "mimi":
            from oracle import mimi_oracle as O

            codes, m = O.rvq_encode(cfg, W, z, K, True)                    # [K, 1, F]
            toks, m = codes[:, 0].t(), m[:, 0].t()
        elif kind == "dac":
            from oracle import dac_oracle as O

            _, codes, m = O.rvq_forward(cfg, W, z, K, return_margin=True)  # [1, K, F]
            toks, m = codes[0].t(), m[0].t()
        else:
            raise ValueError(kind)
    canon = canonical_codes(search_tables(kind, E[:K]))
    toks = torch.stack([canon[k][toks[:, k]] for k in range(K)], 1)
    return toks.contiguous(), m.contiguous()


def cancellation_margins(E: torch.Tensor, x: torch.Tensor, toks: torch.Tensor) -> torch.Tensor:
    """[F, K]: the fp64 gap between the two nearest codes of each stage, (d2 - d1) / (|r|^2 + |e_1|^2), along the chain `toks`.
    The reference computes d = |r|^2 - 2 r.e + |e|^2, so any fp32 evaluation of it errs relative to |r|^2 + |e|^2, not to d:
    a frame that sits much closer to its code than to the origin (trained codebooks: frames and codes share a large common
    component) can have a wide margin relative to d and still be an fp32 near tie.  This is the margin that says so."""
    r = x.double()
    out = []
    for k in range(toks.shape[1]):
        e = E[k].double()
        rr = r.pow(2).sum(1, keepdim=True)
        d = rr - 2 * r @ e.t() + e.pow(2).sum(1)[None]
        two = torch.topk(d, 2, dim=1, largest=False).values
        eb = e[toks[:, k]]
        out.append((two[:, 1] - two[:, 0]) / (rr[:, 0] + eb.pow(2).sum(1)).clamp_min(1e-300))
        r = r - eb
    return torch.stack(out, 1)
