// dnsmos: the P.808 DNSMOS score of a batch of clips -- the arithmetic of downstream/metrics/dnsmos.py:87-152
// (librosa's log-mel front end at its defaults, then a fixed 3x3 conv net) on the device, window by window.
//   * front end (dm_front_kernel): one wave owns 16 frames of one 9 s window.  The 15 * 160 + 352 = 2752 samples those frames cover lie in
//     LDS as split16 planes under ONE power-of-two scale per tile; the window's samples are gathered from the clip with the modulus that
//     stands for the reference's doubling of a short clip, zero outside the window (center = True, constant padding).  The DFT of 321
//     points (K padded to 352 with zero basis rows) is computed TRANSPOSED as in specdist.h, C[bin][frame], 6 passes of 32 bins; the power
//     of every bin goes to LDS in fp32 and the mel product runs from there on the vector pipe: a Slaney filter at 120 mels over 161 bins
//     spans at most 8 bins, so the dense 161 x 120 product would be 98 % zeros, and the sparse sum keeps fp32 over the 80 dB the dB rule
//     looks at (an fp16 pair under one scale per frame does not).  A filter without a bin sums nothing and is exactly 0.
//     The mel power is written once; the window's largest value is an atomicMax on the bits of the non-negative floats: order-independent.
//   * conv5 (dm_conv1_kernel, Cin = 1, vector pipe, fp32): applies the dB rule as it loads, 9 FMAs per output and channel, bias, ReLU and
//     the 2 x 2 max pool in registers; writes channels-last [window][H / 2][W / 2][32].
//   * conv6 .. conv9 (dm_conv_kernel, Cin = 32): an implicit GEMM on the fp16 matrix pipe in split16 arithmetic.  A workgroup of 4 waves
//     owns 8 x 16 output positions; the 10 x 18 x 32 input halo lies in LDS as two fp16 planes under one scale per tile (from the tile's
//     own largest magnitude: no value of another tile or window enters), the 288 x 32 weight image of 32 output channels as fragment
//     images in the lanes' load order (36 KB, loaded once per workgroup; workgroups walk the tiles).  One tap is one k-step of
//     mfma_f32_16x16x32_f16: A = weights (rows: 16 output channels), B = 16 positions (2 rows x 8 columns), so an accumulator lane holds 4
//     consecutive channels of one position and the 2 x 2 pool is two lane exchanges inside a group of 16.  Bias, ReLU and the pool run in the
//     epilogue: the full-resolution output of a pooled layer never reaches memory.  conv9 (64 channels) runs as two halves of 32 and
//     folds the global maximum into the epilogue (atomicMax on the bits of the ReLU's non-negative output).
//   * tail (dm_tail_kernel): the three dense layers, one wave per window, sums in index order.  A window whose mel maximum is not finite
//     (an inf or a NaN in its samples) scores NaN.
//   * dm_mean_kernel: per clip the mean of its windows in order, and the padded [B][Smax] scores.
// Tables (built once by dm_tables_kernel from fp64 values computed on the host, ac_dnsmos_source), basis scale 2^14:
//     basis[6 passes][11 k-steps][2 bin tiles][cos, sin][hi, lo][64 lanes][8 fp16]     lane (i, kq), e: bin 32 pass + 16 tile + i, n = 32 s + 8 kq + e
//     fb   [161][120] fp32, k0[120], k1[120] int32: filter m is fb[k0 .. k1 - 1][m]
// Packed weights (ac_dnsmos_pack, DM_PK_*): conv5 in fp32; conv6 .. conv9 as fragment images
//     [32-channel half][9 taps][2 channel tiles][hi, lo][64 lanes][8 fp16]             lane (i, kq), e: cout 32 half + 16 tile + i, cin 8 kq + e
// with one power-of-two scale per output channel, 2^-scale and the bias behind them; the dense layers in fp32.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "split16.h"

namespace ac {

constexpr int DM_NFFT = 321, DM_HOP = 160, DM_BINS = 161, DM_MELS = 120, DM_FRAMES = 900;
constexpr int DM_WIN = DM_FRAMES * DM_HOP;                     // 144000 samples of a window feed the features
constexpr int DM_FT = 16;                                      // frames per tile (one wave)
constexpr int DM_KS = 11, DM_KPAD = DM_KS * 32;                // 352 >= 321
constexpr int DM_SLAB = (DM_FT - 1) * DM_HOP + DM_KPAD;        // 2752
constexpr int DM_PASSES = 6, DM_PB = DM_PASSES * 32;           // 192 >= 161 bins
constexpr int DM_TILES = (DM_FRAMES + DM_FT - 1) / DM_FT;      // 57
constexpr int DM_S = 14;
constexpr long long DM_BASIS_HALVES = (long long)DM_PASSES * DM_KS * 8 * 512;
constexpr int DM_SRC_COUNT = 2 * DM_NFFT + DM_BINS * DM_MELS;  // fp64 source: cos(2 pi j / 321) [321], sin [321], fb [161][120]
constexpr int DM_MAX_L = 1 << 24;
static_assert(DM_SLAB % 64 == 0, "the slab is loaded by whole waves");

// the flat fp32 weights a caller hands to ac_dnsmos_pack: conv5.w [32][1][3][3], conv5.b, conv6.w [32][32][3][3], conv6.b, conv7, conv8,
// conv9.w [64][32][3][3], conv9.b, dense3.w [64 in][64 out], dense3.b, dense4.w, dense4.b, dense5.w [64][1], dense5.b [1]
constexpr int DM_W_C5 = 0, DM_W_C6 = 320, DM_W_C7 = DM_W_C6 + 9248, DM_W_C8 = DM_W_C7 + 9248, DM_W_C9 = DM_W_C8 + 9248;
constexpr int DM_W_D3 = DM_W_C9 + 18432 + 64, DM_W_COUNT = DM_W_D3 + 4160 + 4160 + 65;
// packed image, byte offsets (all multiples of 16)
constexpr int DM_HALF_HALVES = 9 * 2 * 2 * 512;                // one 32-channel half of a layer: 18432 fp16 = 36 KB
constexpr size_t DM_PK_C5 = 0;                                 // 320 floats
constexpr size_t DM_PK_FRAG = 1280;                            // 5 halves: conv6, conv7, conv8, conv9 low, conv9 high
constexpr size_t DM_PK_WINV = DM_PK_FRAG + (size_t)5 * DM_HALF_HALVES * 2;      // [5][32] floats
constexpr size_t DM_PK_BIAS = DM_PK_WINV + 5 * 32 * 4;                          // [5][32] floats
constexpr size_t DM_PK_DENSE = DM_PK_BIAS + 5 * 32 * 4;                         // 4160 + 4160 + 65 floats
constexpr size_t DM_PK_BYTES = DM_PK_DENSE + (size_t)(4160 + 4160 + 65 + 3) * 4;
static_assert(DM_PK_DENSE % 16 == 0 && DM_PK_BYTES % 16 == 0, "sections keep 16-byte alignment");

constexpr int DM_TY = 8, DM_TX = 16;                           // output positions of a conv tile
constexpr int DM_HY = DM_TY + 2, DM_HX = DM_TX + 2, DM_HPIX = DM_HY * DM_HX;    // 10 x 18 halo
constexpr int DM_HVEC = DM_HPIX * 8;                           // float4 loads of a halo: 1440
constexpr int DM_HREG = (DM_HVEC + 255) / 256;                 // per thread: 6

struct DmTablesParams {
    const double* src;
    _Float16* basis;
    float* fb;
    int* k01;            // [2][120]
};

struct DmPackParams {
    const float* w;      // [DM_W_COUNT]
    unsigned char* pk;
};

struct DmFrontParams {
    const float* sig;        // [B][L]
    const int* plan;         // [S][4]: clip, start, length of the clip (the modulus), index among the clip's windows
    const _Float16* basis;
    const float* fb;
    const int* k01;
    float* melpow;           // [C][900][120]
    unsigned* smax;          // [C]
    long long L;
    int B;
};

struct DmConv1Params {
    const float* feats;      // [C][H][W] or null
    const float* melpow;     // [C][H][W] (when feats is null)
    const unsigned* smax;    // [C]
    const float* w;          // conv5: [32][9], [32]
    float* out;              // [C][H / 2][W / 2][32]
    float* feats_out;        // [C][H][W] or null (melpow mode, even H and W)
    int H, W, C;
};

struct DmConvParams {
    const float* in;         // [C][H][W][32]
    const _Float16* frag;    // first 32-channel half of the layer
    const float* winv;
    const float* bias;
    float* out;              // [C][H or H / 2][W or W / 2][CO] (null with GMAX)
    unsigned* gmax;          // [C][64]
    int H, W, CO, tilesX, tilesY, ntiles;
};

struct DmTailParams {
    const unsigned* gmax;    // [C][64]
    const unsigned* smax;    // [C] or null
    const float* dense;
    float* score;            // [C]
    float* vec_out;          // [C][64] or null
};

struct DmMeanParams {
    const float* seg;        // [S]
    const int* clips;        // [B][2]: first window, number of windows
    float* out;              // [B]
    float* padded;           // [B][Smax] or null
    int B, Smax, S;
};

// Clears the chunk's maxima: a kernel of the library's own, not hipMemsetAsync -- a memset node captured into a hipGraph does not replay
// reliably on this runtime (split16_kernels.h).
__global__ __launch_bounds__(256) void dm_clear_kernel(unsigned* words, int n) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) words[t] = 0u;
}

// One thread per (fragment, lane) of the basis, then one per filterbank value, then one per filter (its range of bins).
__global__ __launch_bounds__(256) void dm_tables_kernel(const DmTablesParams p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nb = (long long)DM_PASSES * DM_KS * 4 * 64, nf = (long long)DM_BINS * DM_MELS;
    if (t < nb) {
        const int lane = (int)(t & 63), i = lane & 15, kq = lane >> 4;
        const int qc = (int)(t >> 6) & 3, s = (int)((t >> 8) % DM_KS), pass = (int)((t >> 8) / DM_KS);
        const int bin = 32 * pass + 16 * (qc >> 1) + i;
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int n = 32 * s + 8 * kq + e;
            double v = 0.0;
            if (bin < DM_BINS && n < DM_NFFT) {
                const int j = (int)(((long long)bin * n) % DM_NFFT);
                v = 0.5 * (1.0 - p.src[n]) * p.src[(qc & 1) ? DM_NFFT + j : j];
            }
            _Float16 h, l;
            s16_split64(v, h, l);
            hi[e] = h;
            lo[e] = l;
        }
        _Float16* o = p.basis + (((long long)(pass * DM_KS + s) * 4 + qc) * 2) * 512 + lane * 8;
        *reinterpret_cast<f16x8*>(o) = hi;
        *reinterpret_cast<f16x8*>(o + 512) = lo;
    } else if (t < nb + nf) {
        p.fb[t - nb] = (float)p.src[2 * DM_NFFT + (t - nb)];
    } else if (t < nb + nf + DM_MELS) {
        const int m = (int)(t - nb - nf);
        int k0 = DM_BINS, k1 = 0;
        for (int k = 0; k < DM_BINS; ++k)
            if ((float)p.src[2 * DM_NFFT + k * DM_MELS + m] != 0.f) {
                k0 = k < k0 ? k : k0;
                k1 = k + 1;
            }
        p.k01[m] = k0 < k1 ? k0 : 0;
        p.k01[DM_MELS + m] = k1;
    }
}

// One thread per (half, tap, channel tile, lane) of the fragment images, then one per remaining fp32 value.
__global__ __launch_bounds__(256) void dm_pack_kernel(const DmPackParams p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int nfrag = 5 * 9 * 2 * 64;
    float* c5 = reinterpret_cast<float*>(p.pk + DM_PK_C5);
    float* dense = reinterpret_cast<float*>(p.pk + DM_PK_DENSE);
    if (t < nfrag) {
        const int lane = t & 63, i = lane & 15, kq = lane >> 4, nt = (t >> 6) & 1, tap = (t >> 7) % 9, half = (t >> 7) / 9;
        const int base = half < 3 ? DM_W_C6 + 9248 * half : DM_W_C9, couts = half < 3 ? 32 : 64;
        const int co = (half == 4 ? 32 : 0) + 16 * nt + i;
        const float* row = p.w + base + co * 288;                // [cin 32][tap 9]
        unsigned am = 0;
        for (int j = 0; j < 288; ++j) amax_acc(am, row[j]);
        const int s = s16_exponent(am, 40);
        const float sc = s16_pow2(s);
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = row[(8 * kq + e) * 9 + tap];
            const _Float16 h = (_Float16)(v * sc);
            hi[e] = h;
            lo[e] = (_Float16)__builtin_fmaf(v, sc, -(float)h);
        }
        _Float16* o = reinterpret_cast<_Float16*>(p.pk + DM_PK_FRAG) + (long long)half * DM_HALF_HALVES + ((tap * 2 + nt) * 2) * 512 + lane * 8;
        *reinterpret_cast<f16x8*>(o) = hi;
        *reinterpret_cast<f16x8*>(o + 512) = lo;
        if (tap == 0 && kq == 0) {
            reinterpret_cast<float*>(p.pk + DM_PK_WINV)[half * 32 + 16 * nt + i] = s16_pow2(-s);
            reinterpret_cast<float*>(p.pk + DM_PK_BIAS)[half * 32 + 16 * nt + i] = p.w[base + couts * 288 + co];
        }
    } else if (t < nfrag + 320) {
        c5[t - nfrag] = p.w[DM_W_C5 + t - nfrag];
    } else if (t < nfrag + 320 + 4160 + 4160 + 65) {
        dense[t - nfrag - 320] = p.w[DM_W_D3 + t - nfrag - 320];
    }
}

// sample j of the window (0 <= j < 144000: the clip read with its modulus; 0 outside: the zero padding of center = True)
__device__ __forceinline__ float dm_sample(const float* clip, int start, int len, int j) {
    return (j >= 0 && j < DM_WIN) ? clip[(start + j) % len] : 0.f;
}

__global__ __launch_bounds__(64) void dm_front_kernel(const DmFrontParams p) {
    __shared__ __attribute__((aligned(16))) _Float16 planes[2][DM_SLAB];
    __shared__ float pw[DM_FT][DM_PB + 1];
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int tile = blockIdx.x, win = blockIdx.y;
    const int* pl = p.plan + 4 * (long long)win;
    // (the plan is the caller's device memory: whatever it holds, no read leaves the signals)
    const int cb = pl[0] < 0 ? 0 : (pl[0] >= p.B ? p.B - 1 : pl[0]);
    const float* clip = p.sig + (long long)cb * p.L;
    const int len = pl[2] < 1 ? 1 : (pl[2] > (int)p.L ? (int)p.L : pl[2]);
    const int start = pl[1] < 0 ? 0 : (pl[1] > DM_MAX_L ? DM_MAX_L : pl[1]);
    const int j0 = tile * DM_FT * DM_HOP - DM_HOP;

    unsigned am = 0;
    for (int c = 0; c < DM_SLAB / 64; ++c) amax_acc(am, dm_sample(clip, start, len, j0 + c * 64 + lane));
    am = group_max_u32<64>(am);
    const int s = s16_exponent(am);
    const float sc = s16_pow2(s), inv = s16_pow2(-(s + DM_S));
    for (int c = 0; c < DM_SLAB / 64; ++c) {
        const int i = c * 64 + lane;
        const float v = dm_sample(clip, start, len, j0 + i);
        const _Float16 h = (_Float16)(v * sc);
        planes[0][i] = h;
        planes[1][i] = (_Float16)__builtin_fmaf(v, sc, -(float)h);
    }
    __syncthreads();

    const f16x8* bt = reinterpret_cast<const f16x8*>(p.basis) + lane;
    const int xo = DM_HOP * li + 8 * kq;
    for (int pass = 0; pass < DM_PASSES; ++pass) {
        s16_f32x4 acc[4];
#pragma unroll
        for (int qc = 0; qc < 4; ++qc) acc[qc] = s16_f32x4{0.f, 0.f, 0.f, 0.f};
        const f16x8* bp = bt + (long long)pass * DM_KS * 8 * 64;
        for (int s2 = 0; s2 < DM_KS; ++s2) {
            f16x8 cur[8];
#pragma unroll
            for (int f = 0; f < 8; ++f) cur[f] = bp[(s2 * 8 + f) * 64];
            const f16x8 xh = *reinterpret_cast<const f16x8*>(&planes[0][xo + 32 * s2]);
            const f16x8 xl = *reinterpret_cast<const f16x8*>(&planes[1][xo + 32 * s2]);
#pragma unroll
            for (int qc = 0; qc < 4; ++qc) acc[qc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[qc * 2], xl, acc[qc], 0, 0, 0);
#pragma unroll
            for (int qc = 0; qc < 4; ++qc) acc[qc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[qc * 2 + 1], xh, acc[qc], 0, 0, 0);
#pragma unroll
            for (int qc = 0; qc < 4; ++qc) acc[qc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[qc * 2], xh, acc[qc], 0, 0, 0);
        }
        // lane (li, kq): frame li, bins 32 pass + 16 t + 4 kq + r
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float re = acc[(e >> 2) * 2][e & 3] * inv, im = acc[(e >> 2) * 2 + 1][e & 3] * inv;
            pw[li][32 * pass + 16 * (e >> 2) + 4 * kq + (e & 3)] = __builtin_fmaf(re, re, im * im);
        }
    }
    __syncthreads();

    unsigned mx = 0;
    for (int it = 0; it < DM_FT * DM_MELS / 64; ++it) {
        const int idx = it * 64 + lane, fr = idx / DM_MELS, m = idx - fr * DM_MELS;
        const int k0 = p.k01[m], k1 = p.k01[DM_MELS + m];
        float a = 0.f;
        for (int k = k0; k < k1; ++k) a = __builtin_fmaf(p.fb[k * DM_MELS + m], pw[fr][k], a);
        const int f = tile * DM_FT + fr;
        if (f < DM_FRAMES) {
            p.melpow[((long long)win * DM_FRAMES + f) * DM_MELS + m] = a;
            const unsigned b = __float_as_uint(__builtin_fabsf(a));      // (an inf or a NaN lies above every finite value)
            mx = b > mx ? b : mx;
        }
    }
    mx = group_max_u32<64>(mx);
    if (lane == 0) atomicMax(p.smax + win, mx);
}

// 10 log10(max(v, 1e-10)), written so that a NaN stays one
__device__ __forceinline__ float dm_db(float v) { return 10.0f * log10f(v < 1e-10f ? 1e-10f : v); }

// the feature of a mel power under the window's maximum: the reference's (power_to_db(S, ref = max) + 40) / 40 with top_db = 80
__device__ __forceinline__ float dm_feature(float v, float ref_db) {
    const float d = dm_db(v) - ref_db;
    return ((d < -80.0f ? -80.0f : d) + 40.0f) / 40.0f;
}

// One thread per pooled position: all 32 channels (the weights are wave-uniform).
__global__ __launch_bounds__(256) void dm_conv1_kernel(const DmConv1Params p) {
#pragma clang fp contract(off)
    const int PH = p.H >> 1, PW = p.W >> 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.C * PH * PW) return;
    const int px = (int)(t % PW), py = (int)((t / PW) % PH), win = (int)(t / ((long long)PW * PH));
    const float* src = (p.feats ? p.feats : p.melpow) + (long long)win * p.H * p.W;
    const float ref_db = p.feats ? 0.f : dm_db(__uint_as_float(p.smax[win]));
    float x[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int y = 2 * py - 1 + a, xx = 2 * px - 1 + b;
            float v = 0.f;
            if (y >= 0 && y < p.H && xx >= 0 && xx < p.W) {
                v = src[(long long)y * p.W + xx];
                if (!p.feats) {
                    v = dm_feature(v, ref_db);
                    if (p.feats_out && a >= 1 && a <= 2 && b >= 1 && b <= 2) p.feats_out[((long long)win * p.H + y) * p.W + xx] = v;
                }
            }
            x[a][b] = v;
        }
    float* o = p.out + t * 32;
    for (int c4 = 0; c4 < 8; ++c4) {
        s16_f32x4 r;
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int c = 4 * c4 + cc;
            const float* w = p.w + 9 * c;
            float best = 0.f;                                     // (ReLU: the pool's maximum is at least 0)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float sum = p.w[288 + c];
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) sum = __builtin_fmaf(w[3 * ky + kx], x[a + ky][b + kx], sum);
                    best = sum > best ? sum : best;
                }
            r[cc] = best;
        }
        *reinterpret_cast<s16_f32x4*>(o + 4 * c4) = r;
    }
}

template <bool POOL, bool GMAX>
__global__ __launch_bounds__(256) void dm_conv_kernel(const DmConvParams p) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) _Float16 wl[DM_HALF_HALVES];
    __shared__ __attribute__((aligned(16))) _Float16 xs[2][DM_HPIX * 32];
    __shared__ unsigned red[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int half = blockIdx.y;
    {
        const f16x8* src = reinterpret_cast<const f16x8*>(p.frag + (long long)half * DM_HALF_HALVES);
        for (int i = tid; i < DM_HALF_HALVES / 8; i += 256) reinterpret_cast<f16x8*>(wl)[i] = src[i];
    }
    float winv[2][4], bias[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            winv[nt][r] = p.winv[half * 32 + 16 * nt + 4 * kq + r];
            bias[nt][r] = p.bias[half * 32 + 16 * nt + 4 * kq + r];
        }
    const int OH = POOL ? p.H >> 1 : p.H, OW = POOL ? p.W >> 1 : p.W;
    const int per = p.tilesX * p.tilesY;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        const int win = tile / per, tr = tile - win * per, ty = tr / p.tilesX, tx = tr - ty * p.tilesX;
        const int y0 = ty * DM_TY, x0 = tx * DM_TX;
        const float* in = p.in + (long long)win * p.H * p.W * 32;
        s16_f32x4 v[DM_HREG];
        unsigned am = 0;
#pragma unroll
        for (int i = 0; i < DM_HREG; ++i) {
            const int idx = tid + 256 * i, pix = idx >> 3, j = idx & 7;
            const int hy = pix / DM_HX, hx = pix - hy * DM_HX, y = y0 - 1 + hy, x = x0 - 1 + hx;
            v[i] = s16_f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < DM_HVEC && y >= 0 && y < p.H && x >= 0 && x < p.W) v[i] = *reinterpret_cast<const s16_f32x4*>(in + ((long long)y * p.W + x) * 32 + 4 * j);
            amax_acc4(am, v[i]);
        }
        am = group_max_u32<64>(am);
        if (lane == 0) red[wv] = am;
        __syncthreads();
        am = red[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) am = red[i] > am ? red[i] : am;
        const int s = s16_exponent(am);
        const float sc = s16_pow2(s), inva = s16_pow2(-s);
#pragma unroll
        for (int i = 0; i < DM_HREG; ++i) {
            const int idx = tid + 256 * i, pix = idx >> 3, j = idx & 7;
            // 8 channels are one 16-byte slot; the slots of a position are permuted by its index so that neighbours spread over the banks
            if (idx < DM_HVEC) split16_store4s(v[i], sc, &xs[0][0], DM_HPIX * 32, pix * 32 + (((j >> 1) ^ (pix & 3)) * 8) + (j & 1) * 4);
        }
        __syncthreads();

        s16_f32x4 acc[2][2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = s16_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap - 3 * ky;
            f16x8 ah[2], al[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                ah[nt] = *reinterpret_cast<const f16x8*>(&wl[((tap * 2 + nt) * 2) * 512 + lane * 8]);
                al[nt] = *reinterpret_cast<const f16x8*>(&wl[((tap * 2 + nt) * 2 + 1) * 512 + lane * 8]);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const int pix = (2 * wv + (li >> 3) + ky) * DM_HX + 8 * mt + (li & 7) + kx;
                const int off = pix * 32 + ((kq ^ (pix & 3)) * 8);
                const f16x8 xh = *reinterpret_cast<const f16x8*>(&xs[0][off]);
                const f16x8 xl = *reinterpret_cast<const f16x8*>(&xs[1][off]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[nt], xl, acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[nt], xh, acc[mt][nt], 0, 0, 0);
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[nt], xh, acc[mt][nt], 0, 0, 0);
                }
            }
        }

        // lane (li, kq): position (2 wv + li / 8, 8 mt + li % 8) of the tile, channels 16 nt + 4 kq + r of the half
        const int y = y0 + 2 * wv + (li >> 3);
        unsigned gm[2][4];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 4; ++r) gm[nt][r] = 0;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int x = x0 + 8 * mt + (li & 7);
            const bool valid = y < p.H && x < p.W;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                s16_f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float val = __builtin_fmaf(acc[mt][nt][r], inva * winv[nt][r], bias[nt][r]);
                    val = val > 0.f ? val : 0.f;
                    if (POOL) {
                        const float a = __shfl_xor(val, 1);
                        val = a > val ? a : val;
                        const float b = __shfl_xor(val, 8);
                        val = b > val ? b : val;
                    }
                    o[r] = val;
                    if (GMAX) {
                        const unsigned bts = valid ? __float_as_uint(val) : 0u;
                        gm[nt][r] = bts > gm[nt][r] ? bts : gm[nt][r];
                    }
                }
                if (!GMAX) {
                    const int co = half * 32 + 16 * nt + 4 * kq;
                    if (POOL) {
                        const int py = y >> 1, px = x >> 1;
                        if (!(li & 9) && py < OH && px < OW) *reinterpret_cast<s16_f32x4*>(p.out + (((long long)win * OH + py) * OW + px) * p.CO + co) = o;
                    } else if (valid) {
                        *reinterpret_cast<s16_f32x4*>(p.out + (((long long)win * OH + y) * OW + x) * p.CO + co) = o;
                    }
                }
            }
        }
        if (GMAX) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned m = group_max_u32<16>(gm[nt][r]);
                    if (li == 0 && m != 0) atomicMax(p.gmax + (long long)win * 64 + half * 32 + 16 * nt + 4 * kq + r, m);
                }
        }
        __syncthreads();      // the next tile's halo overwrites xs and red
    }
}

// One wave per window: the 64 maxima through dense3, dense4 (ReLU) and dense5; every sum runs in index order.
__global__ __launch_bounds__(64) void dm_tail_kernel(const DmTailParams p) {
#pragma clang fp contract(off)
    __shared__ float h[2][64];
    const int lane = threadIdx.x & 63, win = blockIdx.x;
    const float* d3 = p.dense, *d4 = p.dense + 4160, *d5 = p.dense + 8320;
    const float g = __uint_as_float(p.gmax[(long long)win * 64 + lane]);
    if (p.vec_out) p.vec_out[(long long)win * 64 + lane] = g;
    h[0][lane] = g;
    __syncthreads();
    float a = d3[4096 + lane];
    for (int i = 0; i < 64; ++i) a = __builtin_fmaf(h[0][i], d3[i * 64 + lane], a);
    h[1][lane] = a > 0.f ? a : 0.f;
    __syncthreads();
    a = d4[4096 + lane];
    for (int i = 0; i < 64; ++i) a = __builtin_fmaf(h[1][i], d4[i * 64 + lane], a);
    __syncthreads();
    h[0][lane] = a > 0.f ? a : 0.f;
    __syncthreads();
    if (lane == 0) {
        float sc = d5[64];
        for (int i = 0; i < 64; ++i) sc = __builtin_fmaf(h[0][i], d5[i], sc);
        if (p.smax && p.smax[win] >= 0x7f800000u) sc = __uint_as_float(0x7fc00000u);
        p.score[win] = sc;
    }
}

__global__ __launch_bounds__(64) void dm_mean_kernel(const DmMeanParams p) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    int first = p.clips[2 * b], n = p.clips[2 * b + 1];          // (the caller's device memory: clamped, so no read leaves the scores)
    first = first < 0 ? 0 : (first >= p.S ? p.S - 1 : first);
    n = n < 1 ? 1 : (n > p.S - first ? p.S - first : n);
    float a = 0.f;
    for (int i = 0; i < n; ++i) a += p.seg[first + i];
    p.out[b] = a / (float)n;
    if (p.padded)
        for (int i = 0; i < p.Smax; ++i) p.padded[(long long)b * p.Smax + i] = i < n ? p.seg[first + i] : __uint_as_float(0x7fc00000u);
}

}  // namespace ac
