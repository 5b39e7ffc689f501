// knn: cosine k-nearest-neighbour feature matching -- for every query row the k rows of a matching set with the
// largest cosine similarity, and the mean of those rows.  It is the table walk of rvq16.h (one wave owns 16 MS rows, the table streams
// through split16 MFMA tiles, three partial products per k-step) with three differences: the table arrives at run time (knn_pack_kernel
// builds its image on the device), both sides are L2-normalised BEFORE the product, and each lane keeps a sorted list of its best KL
// (similarity, index) pairs per accumulator row where rvq16.h keeps one.
//   * normalising: a row is scaled by the power of two of its largest finite magnitude (s16_exponent: exact, and the squared norm can
//     then neither overflow nor underflow), its squared norm is one fp32 FMA chain per lane and two shuffles, v = x 2^s / sqrt(|x 2^s|^2).
//     |v| <= 1 and the largest element is >= 1 / sqrt(H), so ONE scale, 2^14 (s16_exponent of 1.0), serves every row of both sides.
//     A row is VALID when its largest magnitude is a normal number and its squared norm is finite (no inf / NaN element); every other
//     row -- zero rows, rows of denormals, rows with an inf or a NaN, the padding rows of the last tile -- has zero planes and a zero
//     validity word and can never be matched.
//   * image, the tile order of rvq16.h's epk16 (k-step s of 32, half e of lane (j, kq)  <->  dim 16 (2s + e/4) + 4 kq + e%4):
//         image[Mpad/16 tiles][H/32 k-steps][2 planes][64 lanes][8 fp16],  valid[Mpad] uint32 behind it      (Mpad = 16 ceil(M / 16))
//   * similarity = acc * 2^-28 (exact scaling of the fp32 accumulator): one dot product of unit vectors in split16 arithmetic, the error
//     of an fp32 FMA chain (split16.h) -- NOT the |q|^2 + |t|^2 - cdist^2 form of the reference, which cancels.
//   * order: (similarity descending, index ascending) is a strict total order, and every level applies it -- a lane meets its codes in
//     ascending order and inserts on a strict `>` against its list's tail (the steady state is that one compare, what the argmax costs),
//     the 16 lanes of a row merge by an xor butterfly, the slices of a split walk merge in knn_finish_kernel.  The k best under a total
//     order do not depend on how the set was divided, so every split count returns the same indices, similarities and output bits.
//   * launch form: grid (query tiles, S slices of the table's tiles); every workgroup writes its rows' KL best to the workspace
//     ws_sim / ws_idx [Q][S][KL]; knn_finish_kernel (one wave per query row) merges the S lists, gathers the k = min(topk, valid rows)
//     ORIGINAL fp32 rows, sums them nearest first, multiplies by 1 / k and writes the row, its indices and its similarities.  S = 1 is
//     the same two launches with nothing to merge.  A query row that is not valid owns an empty list: NaN output, indices -1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "split16.h"

namespace ac {

constexpr int KNN_MAX_TOPK = 8;
constexpr int KNN_MAX_SPLITS = 64;
constexpr int KNN_MAX_ROWS = 1 << 24;      // rows of either side: tile offsets (rows * H * 2 halves) are 64-bit, row indices stay far inside int32
constexpr int KNN_NONE = 0x7fffffff;       // index of an empty list entry (similarity -inf): behind every real entry in the order
constexpr int KNN_S = 14;                  // s16_exponent(bits of 1.0f): |v| <= 1  ->  |v| 2^14 < 2^15

struct KnnPackParams {
    const float* set;        // [M][H]
    _Float16* image;         // layout above
    unsigned* valid;         // [Mpad]
    int M, H;
};

struct KnnMatchParams {
    const float* query;      // [Q][H]
    const _Float16* image;
    const unsigned* valid;
    float* ws_sim;           // [Q][S][KL]
    int* ws_idx;             // [Q][S][KL]
    int Q, ctiles, S;
};

struct KnnFinishParams {
    const float* set;        // [M][H], the ORIGINAL rows
    const float* ws_sim;
    const int* ws_idx;
    float* out;              // [Q][H] or null
    long long* idx;          // [Q][topk] or null: nearest first, -1 behind k
    float* sim;              // [Q][topk] or null: cosine similarity, NaN behind k
    int Q, H, S, topk;
};

// the power-of-two scale of a row from its largest finite magnitude, and whether that magnitude is a normal number
__device__ __forceinline__ float knn_row_scale(unsigned am, bool& normal) {
    normal = am >= 0x00800000u;
    return s16_pow2(s16_exponent(am));
}

// (s, i) into a list sorted by (similarity descending, index ascending).  TIE = false is the walk's form: the caller's indices ascend, so
// a candidate equal to an entry belongs behind it and a strict compare against the tail decides.
template <int KL, bool TIE>
__host__ __device__ __forceinline__ void knn_insert(float (&ls)[KL], int (&lx)[KL], float s, int i) {
    const bool in = TIE ? (s > ls[KL - 1] || (s == ls[KL - 1] && i < lx[KL - 1])) : s > ls[KL - 1];
    if (in) {
        ls[KL - 1] = s;
        lx[KL - 1] = i;
#pragma unroll
        for (int j = KL - 1; j > 0; --j) {
            const bool up = TIE ? (ls[j] > ls[j - 1] || (ls[j] == ls[j - 1] && lx[j] < lx[j - 1])) : ls[j] > ls[j - 1];
            const float ts = ls[j - 1];
            const int ti = lx[j - 1];
            ls[j - 1] = up ? ls[j] : ts;
            lx[j - 1] = up ? lx[j] : ti;
            ls[j] = up ? ts : ls[j];
            lx[j] = up ? ti : lx[j];
        }
    }
}

// One wave per tile of 16 rows; lane (li, kq) holds row li's dims 16 v + 4 kq .. + 3 like a lane of the match kernel.  Three passes over
// the row (largest magnitude, squared norm, planes): the second and third come from the cache.
__global__ __launch_bounds__(64) void knn_pack_kernel(const KnnPackParams p) {
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int HV = p.H / 16, KS = p.H / 32;
    const long long tile = blockIdx.x;
    const long long row = tile * 16 + li;
    const bool inside = row < p.M;
    const float* xr = p.set + (inside ? row : 0) * p.H + 4 * kq;
    unsigned am = 0;
    for (int v = 0; v < HV; ++v) {
        const s16_f32x4 a = inside ? *reinterpret_cast<const s16_f32x4*>(xr + v * 16) : s16_f32x4{0.f, 0.f, 0.f, 0.f};
        amax_acc4(am, a);
    }
    unsigned t = (unsigned)__shfl_xor((int)am, 16);
    am = t > am ? t : am;
    t = (unsigned)__shfl_xor((int)am, 32);
    am = t > am ? t : am;
    bool normal;
    const float sc = knn_row_scale(am, normal);
    float xx = 0.f;
    for (int v = 0; v < HV; ++v) {
        s16_f32x4 a = inside ? *reinterpret_cast<const s16_f32x4*>(xr + v * 16) : s16_f32x4{0.f, 0.f, 0.f, 0.f};
        a = a * sc;
        xx = fmaf(a.x, a.x, xx); xx = fmaf(a.y, a.y, xx); xx = fmaf(a.z, a.z, xx); xx = fmaf(a.w, a.w, xx);
    }
    xx += __shfl_xor(xx, 16);
    xx += __shfl_xor(xx, 32);
    const bool ok = inside && normal && xx > 0.f && xx < __builtin_inff();
    const float inv = ok ? 1.0f / sqrtf(xx) : 0.f;
    const float sx = s16_pow2(KNN_S);
    _Float16* it = p.image + tile * KS * 1024 + lane * 8;
    for (int s = 0; s < KS; ++s) {
        s16_f32x4 a = s16_f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
        if (ok) {
            a = *reinterpret_cast<const s16_f32x4*>(xr + (2 * s) * 16);
            b = *reinterpret_cast<const s16_f32x4*>(xr + (2 * s + 1) * 16);
        }
        const float v8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = (v8[e] * sc) * inv;
            const _Float16 h = (_Float16)(v * sx);
            hi[e] = h;
            lo[e] = (_Float16)__builtin_fmaf(v, sx, -(float)h);
        }
        *reinterpret_cast<f16x8*>(it + (long long)(s * 2 + 0) * 512) = hi;
        *reinterpret_cast<f16x8*>(it + (long long)(s * 2 + 1) * 512) = lo;
    }
    if (kq == 0) p.valid[row] = ok ? 1u : 0u;
}

// HV = H / 16, MS row tiles per wave, KL list length (4 or 8: topk rounded up)
template <int HV, int MS, int KL>
__global__ __launch_bounds__(64) void knn_match_kernel(const KnnMatchParams p) {
    static_assert(HV % 2 == 0, "k-steps of 32 dims");
    constexpr int KS = HV / 2;
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * (16 * MS);
    const int H = HV * 16;
    const float sx = s16_pow2(KNN_S);

    f16x8 xh[MS][KS], xl[MS][KS];
    int qok[MS];
#pragma unroll
    for (int m = 0; m < MS; ++m) {
        const int qrow = q0 + m * 16 + li;
        s16_f32x4 res[HV];
#pragma unroll
        for (int v = 0; v < HV; ++v)
            res[v] = qrow < p.Q ? *reinterpret_cast<const s16_f32x4*>(p.query + (long long)qrow * H + v * 16 + 4 * kq) : s16_f32x4{0.f, 0.f, 0.f, 0.f};
        unsigned am = 0;
#pragma unroll
        for (int v = 0; v < HV; ++v) amax_acc4(am, res[v]);
        unsigned t = (unsigned)__shfl_xor((int)am, 16);
        am = t > am ? t : am;
        t = (unsigned)__shfl_xor((int)am, 32);
        am = t > am ? t : am;
        bool normal;
        const float sc = knn_row_scale(am, normal);
        float xx = 0.f;
#pragma unroll
        for (int v = 0; v < HV; ++v) {
            res[v] = res[v] * sc;
            xx = fmaf(res[v].x, res[v].x, xx); xx = fmaf(res[v].y, res[v].y, xx);
            xx = fmaf(res[v].z, res[v].z, xx); xx = fmaf(res[v].w, res[v].w, xx);
        }
        xx += __shfl_xor(xx, 16);
        xx += __shfl_xor(xx, 32);
        const bool ok = normal && xx > 0.f && xx < __builtin_inff();     // (a row that is not valid walks with zero planes and is emptied below)
        const float inv = ok ? 1.0f / sqrtf(xx) : 0.f;
        qok[m] = ok ? 1 : 0;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const s16_f32x4 a = res[2 * s], b = res[2 * s + 1];
            const float v8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = ok ? v8[e] * inv : 0.f;
                const _Float16 h = (_Float16)(v * sx);
                xh[m][s][e] = h;
                xl[m][s][e] = (_Float16)__builtin_fmaf(v, sx, -(float)h);
            }
        }
    }

    float ls[MS][4][KL];
    int lx[MS][4][KL];
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < KL; ++j) { ls[m][r][j] = -__builtin_inff(); lx[m][r][j] = KNN_NONE; }

    // this slice's tiles: [t0, t1) of the table's ctiles (an empty slice writes empty lists)
    const int t0 = (int)((long long)p.ctiles * blockIdx.y / p.S), t1 = (int)((long long)p.ctiles * (blockIdx.y + 1) / p.S);
    const _Float16* ep = p.image + lane * 8;
    auto load_tile = [&](int ct, f16x8 (&bh)[KS], f16x8 (&bl)[KS], unsigned& vld) {
        const _Float16* et = ep + (long long)ct * KS * 1024;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            bh[s] = *reinterpret_cast<const f16x8*>(et + (s * 2 + 0) * 512);
            bl[s] = *reinterpret_cast<const f16x8*>(et + (s * 2 + 1) * 512);
        }
        vld = p.valid[ct * 16 + li];
    };
    auto run_tile = [&](int ct, const f16x8 (&bh)[KS], const f16x8 (&bl)[KS], bool live) {
        s16_f32x4 acc[MS];
#pragma unroll
        for (int m = 0; m < MS; ++m) acc[m] = s16_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
#pragma unroll
            for (int m = 0; m < MS; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl[m][s], bh[s], acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MS; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[m][s], bl[s], acc[m], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < MS; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh[m][s], bh[s], acc[m], 0, 0, 0);
        }
        const int code = ct * 16 + li;
#pragma unroll
        for (int m = 0; m < MS; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = live ? acc[m][r] * 0x1p-28f : -__builtin_inff();      // exact: a power of two
                knn_insert<KL, false>(ls[m][r], lx[m][r], s, code);
            }
    };
    if (t0 < t1) {       // two tile sets in registers: tile ct + 1 travels under tile ct's MFMAs; the look-ahead past the end re-reads a tile that is not live
        f16x8 bh0[KS], bl0[KS], bh1[KS], bl1[KS];
        unsigned v0, v1;
        load_tile(t0, bh0, bl0, v0);
        for (int ct = t0; ct < t1; ct += 2) {
            const bool second = ct + 1 < t1;
            load_tile(second ? ct + 1 : ct, bh1, bl1, v1);
            run_tile(ct, bh0, bl0, v0 != 0);
            load_tile(ct + 2 < t1 ? ct + 2 : ct, bh0, bl0, v0);
            run_tile(ct + 1, bh1, bl1, second && v1 != 0);
        }
    }

    // the 16 lanes of a row (same kq) hold disjoint lists: an xor butterfly leaves the row's KL best, in order, in every one of them
#pragma unroll
    for (int m = 0; m < MS; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int sh = 1; sh < 16; sh <<= 1) {
                float os[KL];
                int ox[KL];
#pragma unroll
                for (int j = 0; j < KL; ++j) { os[j] = __shfl_xor(ls[m][r][j], sh); ox[j] = __shfl_xor(lx[m][r][j], sh); }
#pragma unroll
                for (int j = 0; j < KL; ++j) knn_insert<KL, true>(ls[m][r], lx[m][r], os[j], ox[j]);
            }
        }
    // rows 4 kq + r of tile m: the lane with li == 0 writes them.  A query row that is not valid (its flag sits in the lanes li = row) owns nothing.
#pragma unroll
    for (int m = 0; m < MS; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rowok = __shfl(qok[m], kq * 4 + r);
            const int qrow = q0 + m * 16 + kq * 4 + r;
            if (li == 0 && qrow < p.Q) {
                const long long o = ((long long)qrow * p.S + blockIdx.y) * KL;
#pragma unroll
                for (int j = 0; j < KL; ++j) {
                    p.ws_sim[o + j] = rowok ? ls[m][r][j] : -__builtin_inff();
                    p.ws_idx[o + j] = rowok ? lx[m][r][j] : KNN_NONE;
                }
            }
        }
    }
}

// One wave per query row: the S lists of the row merge under the same order (every lane computes the same list: the loads broadcast),
// then lane l gathers dims 4 l .. 4 l + 3 (+ 256 per pass) of the k original rows, nearest first.
template <int KL>
__global__ __launch_bounds__(64) void knn_finish_kernel(const KnnFinishParams p) {
    const int lane = threadIdx.x & 63;
    const long long row = blockIdx.x;
    float bs[KL];
    int bi[KL];
#pragma unroll
    for (int j = 0; j < KL; ++j) { bs[j] = -__builtin_inff(); bi[j] = KNN_NONE; }
    const float* ws = p.ws_sim + row * p.S * KL;
    const int* wi = p.ws_idx + row * p.S * KL;
    for (int c = 0; c < p.S * KL; ++c) knn_insert<KL, true>(bs, bi, ws[c], wi[c]);
    int k = 0;
#pragma unroll
    for (int j = 0; j < KL; ++j) k += (j < p.topk && bi[j] != KNN_NONE) ? 1 : 0;
    if (lane < p.topk) {
        int mine = KNN_NONE;
        float ms = 0.f;
#pragma unroll
        for (int j = 0; j < KL; ++j)
            if (j == lane) { mine = bi[j]; ms = bs[j]; }
        const bool have = lane < k;
        if (p.idx) p.idx[row * p.topk + lane] = have ? (long long)mine : -1ll;
        if (p.sim) p.sim[row * p.topk + lane] = have ? ms : __builtin_nanf("");
    }
    if (!p.out) return;
    const float rk = k > 0 ? 1.0f / (float)k : __builtin_nanf("");
    for (int h = lane * 4; h < p.H; h += 256) {
        s16_f32x4 a = s16_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KL; ++j)
            if (j < k) {
                const s16_f32x4 t = *reinterpret_cast<const s16_f32x4*>(p.set + (long long)bi[j] * p.H + h);
                a = j == 0 ? t : a + t;
            }
        *reinterpret_cast<s16_f32x4*>(p.out + row * p.H + h) = a * rk;
    }
}

}  // namespace ac
