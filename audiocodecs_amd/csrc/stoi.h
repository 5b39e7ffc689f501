// stoi: the short-time objective intelligibility of a decoded batch against its reference -- the arithmetic of
// downstream/metrics/stoi.py (torchmetrics -> pystoi at its defaults, extended = False) from the 10 kHz signals on: silent-frame removal,
// overlap-add, STFT, 15 third-octave band envelopes, the clipped and normalised correlation over sliding segments of 30 frames.  The
// REFERENCE is pystoi's x: it alone decides the silent frames, the clipping bound and the normalisation target.  Nothing is read back
// by the host: K, the number of kept frames, stays on the device, grids are sized from F0 (the frames before removal) and workgroups
// whose tile lies past K - 1 exit.  Four launches behind the two FIR launches (ac_resample with the bank of ac_stoi_tables):
//   * stoi_mask_kernel, one workgroup per (clip, signal).  Signal 0 (the reference): frame energies e_f = 20 log10(||w x_f|| + 2^-52), one
//     wave per frame; the clip's maximum; kept_f = e_f > max - 40; an exclusive scan by ballots, 256 frames a step, gives the source-frame
//     list src[0 .. K) and K.  Every signal: a flag if any of its 10 kHz samples (or a reference energy) is not finite -- such a clip gets
//     a NaN score whichever frames the rule happens to keep.
//   * stoi_bands_kernel, one workgroup of four waves per (clip, tile of 16 STFT frames of the rebuilt signal), for ALL 1 + P signals of
//     the clip: the mask, the list and the reference's planes are shared by the hypotheses.  The 17 half-blocks of 128 samples the
//     tile's frames cover are gathered through src -- half-block j = w[128 + n] s[128 src(j - 1) + 128 + n] + w[n] s[128 src(j) + n], one
//     term only at the two ends -- scaled by ONE power of two per signal and tile (amax_acc, s16_exponent) and laid into LDS as split16
//     planes, a half-block every 136 halves so that the 16 frames of an A fragment fall into different banks.  The DFT is
//     C[frame][bin] = sum_n x[frame][n] (w[n] trig(2 pi bin n / 512)), K = 256: the frames are the A operand, the basis the B operand.
//     The basis columns are ordered BY BAND: each of the 22 column tiles holds up to 16 bins of one band (zero columns fill it), so the
//     band sum of |X|^2 is the sum over the 16 lanes of a row of the accumulator tile -- an xor butterfly, fp32, no second product and
//     no spectrum anywhere.  A wave keeps the 32 basis fragments of its tile in registers and multiplies every signal of the clip with
//     them; per (signal, tile, frame) one partial sum goes to LDS, the bands that span two or three tiles are added in tile order, the
//     square root of the sum is the envelope: 16 floats per (signal, clip, frame) reach the workspace (the 16th is 0).
//   * stoi_segments_kernel, one workgroup per (hypothesis, clip, 16 segments): 16 lanes a segment, one per band; every (segment, band) is
//     a direct 30-term computation from the envelopes -- no running window sums.  The 15 correlations of a segment are added by a butterfly.
//   * stoi_finish_kernel, one wave per (hypothesis, clip): lane l adds segments l, l + 64, ... in order, the 64 sums fold by an xor
//     butterfly -- an order that depends on K alone -- and the sum is divided by 15 S.  K - 1 < 30 gives 1e-5 (pystoi's warning path).
// A clip's bits depend on nothing else in the call: every workgroup reads one clip, and a hypothesis' values do not depend on how many
// hypotheses share the workgroup.
//   tables (built once by stoi_tables_kernel from fp64 values computed on the host, ac_stoi_source):
//         window[256] fp32 | fir[5 phases][123 taps] fp32 (ac_resample's layout, width 58) | basis, scale 2^14:
//         basis[22 tiles][8 k-steps][cos, sin][hi, lo][64 lanes][8 fp16]     lane (i, kq), e: bin ST_TILE_BIN0[tile] + i, n = 32 s + 8 kq + e
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "split16.h"

namespace ac {

constexpr int ST_WIN = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_FT = 16;                                       // STFT frames per tile
constexpr int ST_HB = ST_FT + 1;                                // half-blocks a tile's frames cover
constexpr int ST_HB_STRIDE = ST_HOP + 8;                        // halves between half-blocks in LDS (272 bytes: 16 frames, 16 different bank groups)
constexpr int ST_SLAB = ST_HB * ST_HB_STRIDE;
constexpr int ST_TILES = 22, ST_KS = ST_WIN / 32;
constexpr int ST_MAX_P = 4, ST_MAX_SIG = ST_MAX_P + 1;
constexpr int ST_MAX_L16 = 1 << 24;
constexpr int ST_UP = 5, ST_DOWN = 8, ST_FIR_HALF = 290, ST_FIR_TAPS = 123, ST_FIR_WIDTH = 58;
constexpr int ST_SRC_COUNT = ST_WIN + ST_NFFT + 2 * ST_FIR_HALF + 1;      // fp64 source: window [256], cos(2 pi j / 512) [512], h [581]
constexpr long long ST_BASIS_HALVES = (long long)ST_TILES * ST_KS * 4 * 512;
constexpr size_t ST_WINDOW_BYTES = ST_WIN * sizeof(float);
constexpr size_t ST_FIR_BYTES = (size_t)((ST_UP * ST_FIR_TAPS * sizeof(float) + 15) / 16 * 16);
constexpr float ST_EPS = 2.220446049250313e-16f;                // 2^-52
constexpr float ST_CLIP = 6.623413251903491f;                   // 1 + 10^(15 / 20)

// Third-octave bands: the bins [lo, hi) nearest 150 * 2^((2 k -+ 1) / 6) Hz on the grid of 10000 / 512 Hz, and their column tiles
__device__ const short ST_BAND_LO[ST_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
__device__ const short ST_BAND_TILE0[ST_BANDS + 2] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 19, 22, 22};      // (band 15 is the empty 16th column of the envelopes)
__device__ const short ST_TILE_BAND[ST_TILES] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 10, 11, 11, 12, 12, 13, 13, 13, 14, 14, 14};
__device__ const short ST_TILE_BIN0[ST_TILES] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 85, 87, 103, 109, 125, 138, 154, 170, 174, 190, 206};

struct StTablesParams {
    const double* src;       // [ST_SRC_COUNT]
    float* window;           // [256]
    float* fir;              // [5][123]
    _Float16* basis;
};

struct StMaskParams {
    const float* x10;        // [1 + P][B][L10]
    const float* window;
    float* energy;           // [B][F0]
    int* src;                // [B][F0]
    int* K;                  // [B]
    int* bad;                // [1 + P][B]
    uint8_t* kept;           // [B][F0]
    uint8_t* kept_out;       // [B][F0] or null
    int* nseg_out;           // [B] or null
    int B, L10, F0;
};

struct StBandsParams {
    const float* x10;
    const float* window;
    const _Float16* basis;
    const int* src;
    const int* K;
    float* env;              // [1 + P][B][F0][16]
    int B, L10, F0, tiles, nsig;
};

struct StSegParams {
    const float* env;
    const int* K;
    float* segsum;           // [P][B][NS0]: per segment the sum of the 15 band correlations
    int B, F0, NS0, chunks;
};

struct StFinishParams {
    const float* segsum;
    const int* K;
    const int* bad;
    float* score;            // [P][B]
    float* segments_out;     // [P][B][NS0] or null
    int B, NS0;
};

__global__ __launch_bounds__(256) void stoi_tables_kernel(const StTablesParams p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int nb = ST_TILES * ST_KS * 2 * 64;
    if (t < nb) {
        const int lane = t & 63, i = lane & 15, kq = lane >> 4, c = (t >> 6) & 1, s = (t >> 7) & 7, tile = t >> 10;
        const int bin = ST_TILE_BIN0[tile] + i;
        const bool live = bin < ST_BAND_LO[ST_TILE_BAND[tile] + 1];
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int n = 32 * s + 8 * kq + e;
            const int j = (bin * n) & (ST_NFFT - 1);
            const double v = live ? p.src[n] * p.src[ST_WIN + (c ? ((j + 384) & (ST_NFFT - 1)) : j)] : 0.0;      // sin a = cos(a - pi / 2)
            _Float16 h, l;
            s16_split64(v, h, l);
            hi[e] = h;
            lo[e] = l;
        }
        _Float16* o = p.basis + ((long long)((tile * ST_KS + s) * 2 + c) * 2) * 512 + lane * 8;
        *reinterpret_cast<f16x8*>(o) = hi;
        *reinterpret_cast<f16x8*>(o + 512) = lo;
        return;
    }
    const int u = t - nb;
    if (u < ST_WIN) {
        p.window[u] = (float)p.src[u];
    } else if (u < ST_WIN + ST_UP * ST_FIR_TAPS) {
        const int ph = (u - ST_WIN) / ST_FIR_TAPS, jj = (u - ST_WIN) % ST_FIR_TAPS;
        const int k = ST_FIR_HALF + ST_DOWN * ph - ST_UP * (jj - ST_FIR_WIDTH);
        p.fir[u - ST_WIN] = (k >= 0 && k <= 2 * ST_FIR_HALF) ? (float)p.src[ST_WIN + ST_NFFT + k] : 0.f;
    }
}

__device__ __forceinline__ bool st_finite(float v) { return __builtin_amdgcn_classf(v, 0x1F8); }      // +-normal, +-subnormal, +-0

__global__ __launch_bounds__(256) void stoi_mask_kernel(const StMaskParams p) {
    __shared__ float wred[4];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x, g = blockIdx.y;
    const float* x = p.x10 + ((long long)g * p.B + b) * p.L10;
    int notfinite = 0;
    for (int i = tid; i < p.L10; i += 256) notfinite |= !st_finite(x[i]);
    if (g != 0) {
        notfinite = __syncthreads_or(notfinite);
        if (tid == 0) p.bad[(long long)g * p.B + b] = notfinite;
        return;
    }
    float* en = p.energy + (long long)b * p.F0;
    const float w0 = p.window[lane], w1 = p.window[lane + 64], w2 = p.window[lane + 128], w3 = p.window[lane + 192];
    float mx = -INFINITY;
    for (int f = wave; f < p.F0; f += 4) {
        const float* xf = x + (long long)f * ST_HOP + lane;
        const float a0 = w0 * xf[0], a1 = w1 * xf[64], a2 = w2 * xf[128], a3 = w3 * xf[192];
        float ss = (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) ss += __shfl_xor(ss, sh);
        const float e = 20.0f * log10f(sqrtf(ss) + ST_EPS);
        notfinite |= !st_finite(e);
        mx = e > mx ? e : mx;
        if (lane == 0) en[f] = e;
    }
    if (lane == 0) wred[wave] = mx;
    notfinite = __syncthreads_or(notfinite);      // (also: the energies and wred are visible to the workgroup)
    mx = wred[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) mx = wred[w] > mx ? wred[w] : mx;
    const float thr = mx - 40.0f;
    int* src = p.src + (long long)b * p.F0;
    int base = 0;
    for (int c0 = 0; c0 < p.F0; c0 += 256) {
        const int f = c0 + tid;
        const bool k = f < p.F0 && en[f] > thr;
        const unsigned long long bal = __ballot(k);
        if (lane == 0) wcnt[wave] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            off += w < wave ? wcnt[w] : 0;
            tot += wcnt[w];
        }
        if (k) src[off + __popcll(bal & ((1ull << lane) - 1ull))] = f;
        if (f < p.F0) {
            p.kept[(long long)b * p.F0 + f] = k;
            if (p.kept_out) p.kept_out[(long long)b * p.F0 + f] = k;
        }
        base += tot;
        __syncthreads();
    }
    if (tid == 0) {
        p.K[b] = base;
        p.bad[b] = notfinite;
        if (p.nseg_out) p.nseg_out[b] = base > ST_SEG ? base - ST_SEG : 0;
    }
}

// element idx (half-block j = idx / 128, sample n = idx % 128) of a tile's slab of the rebuilt signal
__device__ __forceinline__ float st_rebuilt(const float* sig, const float* window, const int* srcl, int idx) {
#pragma clang fp contract(off)
    const int j = idx >> 7, n = idx & 127;
    const int fa = srcl[j], fb = srcl[j + 1];      // source frames of half-blocks' owners: rebuilt frames (first + j - 1) and (first + j); -1: none
    const float a = fa >= 0 ? window[ST_HOP + n] * sig[(long long)fa * ST_HOP + ST_HOP + n] : 0.f;
    const float c = fb >= 0 ? window[n] * sig[(long long)fb * ST_HOP + n] : 0.f;
    return a + c;
}

__global__ __launch_bounds__(256) void stoi_bands_kernel(const StBandsParams p) {
    __shared__ __attribute__((aligned(16))) _Float16 planes[ST_MAX_SIG][2][ST_SLAB];      // [signal][hi, lo][half-block * 136 + sample]
    __shared__ float part[ST_MAX_SIG][ST_TILES][ST_FT];
    __shared__ unsigned wmax[ST_MAX_SIG][4];
    __shared__ int srcl[ST_HB + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles), b = (int)(blockIdx.x / (unsigned)p.tiles);
    const int K = p.K[b], f0 = tile * ST_FT;
    if (f0 >= K - 1) return;                         // (uniform: the whole workgroup leaves before any barrier)
    if (tid < ST_HB + 1) {
        const int f = f0 + tid - 1;                  // rebuilt frame whose halves make up half-blocks f0 + tid - 1 (second half) and f0 + tid (first half)
        srcl[tid] = (f >= 0 && f < K) ? p.src[(long long)b * p.F0 + f] : -1;
    }
    __syncthreads();
    for (int g = 0; g < p.nsig; ++g) {
        const float* sig = p.x10 + ((long long)g * p.B + b) * p.L10;
        unsigned am = 0;
        for (int idx = tid; idx < ST_HB * ST_HOP; idx += 256) amax_acc(am, st_rebuilt(sig, p.window, srcl, idx));
        am = group_max_u32<64>(am);
        if (lane == 0) wmax[g][wave] = am;
    }
    __syncthreads();
    for (int g = 0; g < p.nsig; ++g) {
        const float* sig = p.x10 + ((long long)g * p.B + b) * p.L10;
        unsigned am = wmax[g][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) am = wmax[g][w] > am ? wmax[g][w] : am;
        const float sc = s16_pow2(s16_exponent(am));
        for (int idx = tid; idx < ST_HB * ST_HOP; idx += 256) {
            const float v = st_rebuilt(sig, p.window, srcl, idx);
            const int o = (idx >> 7) * ST_HB_STRIDE + (idx & 127);
            const _Float16 h = (_Float16)(v * sc);
            planes[g][0][o] = h;
            planes[g][1][o] = (_Float16)__builtin_fmaf(v, sc, -(float)h);
        }
    }
    __syncthreads();

    const f16x8* bt = reinterpret_cast<const f16x8*>(p.basis) + lane;
    for (int ct = wave; ct < ST_TILES; ct += 4) {
        f16x8 bf[ST_KS][4];                          // [k-step][cos hi, cos lo, sin hi, sin lo]
#pragma unroll
        for (int s = 0; s < ST_KS; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) bf[s][q] = bt[((ct * ST_KS + s) * 4 + q) * 64];
        for (int g = 0; g < p.nsig; ++g) {
            unsigned am = wmax[g][0];
#pragma unroll
            for (int w = 1; w < 4; ++w) am = wmax[g][w] > am ? wmax[g][w] : am;
            const float inv = s16_pow2(-(s16_exponent(am) + 14));
            s16_f32x4 ac = {0.f, 0.f, 0.f, 0.f}, as = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < ST_KS; ++s) {
                const int k = 32 * s + 8 * kq;
                const int o = (li + (k >> 7)) * ST_HB_STRIDE + (k & 127);
                const f16x8 xh = *reinterpret_cast<const f16x8*>(&planes[g][0][o]);
                const f16x8 xl = *reinterpret_cast<const f16x8*>(&planes[g][1][o]);
                ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, bf[s][0], ac, 0, 0, 0);
                as = __builtin_amdgcn_mfma_f32_16x16x32_f16(xl, bf[s][2], as, 0, 0, 0);
                ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bf[s][1], ac, 0, 0, 0);
                as = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bf[s][3], as, 0, 0, 0);
                ac = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bf[s][0], ac, 0, 0, 0);
                as = __builtin_amdgcn_mfma_f32_16x16x32_f16(xh, bf[s][2], as, 0, 0, 0);
            }
            // this lane: bin column li of the tile, frames 4 kq .. 4 kq + 3.  The band's part in this tile: the sum over the 16 columns.
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float re = ac[r] * inv, im = as[r] * inv;
                float pw = __builtin_fmaf(re, re, im * im);
#pragma unroll
                for (int sh = 1; sh < 16; sh <<= 1) pw += __shfl_xor(pw, sh);
                if (li == 0) part[g][ct][4 * kq + r] = pw;
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < p.nsig * ST_FT * 16; t += 256) {
        const int band = t & 15, fr = (t >> 4) & 15, g = t >> 8;
        const int f = f0 + fr;
        if (f >= K - 1) continue;
        float s = 0.f;
        for (int ct = ST_BAND_TILE0[band]; ct < ST_BAND_TILE0[band + 1]; ++ct) s += part[g][ct][fr];
        p.env[(((long long)g * p.B + b) * p.F0 + f) * 16 + band] = sqrtf(s);
    }
}

__global__ __launch_bounds__(256) void stoi_segments_kernel(const StSegParams p) {
    const int tid = threadIdx.x, band = tid & 15;
    const int chunk = (int)(blockIdx.x % (unsigned)p.chunks), pb = (int)(blockIdx.x / (unsigned)p.chunks);      // pb = hypothesis * B + clip
    const int b = pb % p.B;
    const int K = p.K[b], S = K - ST_SEG;            // segments 0 .. S - 1; segment i holds the frames i .. i + 29
    const int i = chunk * 16 + (tid >> 4);
    if (chunk * 16 >= S) return;
    const bool live = i < S && band < ST_BANDS;
    float corr = 0.f;
    if (live) {
        const float* ex = p.env + (((long long)b) * p.F0 + i) * 16 + band;
        const float* ey = p.env + (((long long)p.B + pb) * p.F0 + i) * 16 + band;
        float x[ST_SEG], y[ST_SEG];
        float nx = 0.f, ny = 0.f;
#pragma unroll
        for (int n = 0; n < ST_SEG; ++n) {
            x[n] = ex[n * 16];
            y[n] = ey[n * 16];
            nx = __builtin_fmaf(x[n], x[n], nx);
            ny = __builtin_fmaf(y[n], y[n], ny);
        }
        const float c = sqrtf(nx) / (sqrtf(ny) + ST_EPS);
        float mx = 0.f, my = 0.f;
#pragma unroll
        for (int n = 0; n < ST_SEG; ++n) {
            const float cy = c * y[n], bound = x[n] * ST_CLIP;
            y[n] = !(cy >= bound) ? cy : bound;      // min that keeps a NaN
            mx += x[n];
            my += y[n];
        }
        mx *= 1.0f / ST_SEG;
        my *= 1.0f / ST_SEG;
        float vx = 0.f, vy = 0.f;
#pragma unroll
        for (int n = 0; n < ST_SEG; ++n) {
            x[n] -= mx;
            y[n] -= my;
            vx = __builtin_fmaf(x[n], x[n], vx);
            vy = __builtin_fmaf(y[n], y[n], vy);
        }
        const float ix = 1.0f / (sqrtf(vx) + ST_EPS), iy = 1.0f / (sqrtf(vy) + ST_EPS);
#pragma unroll
        for (int n = 0; n < ST_SEG; ++n) corr = __builtin_fmaf(x[n] * ix, y[n] * iy, corr);
    }
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) corr += __shfl_xor(corr, sh);
    if (band == 0 && i < S) p.segsum[(long long)pb * p.NS0 + i] = corr;
}

__global__ __launch_bounds__(64) void stoi_finish_kernel(const StFinishParams p) {
    const int lane = threadIdx.x & 63, pb = blockIdx.x, b = pb % p.B;
    const int K = p.K[b], S = K > ST_SEG ? K - ST_SEG : 0;
    const float* ss = p.segsum + (long long)pb * p.NS0;
    float a = 0.f;
    for (int i = lane; i < S; i += 64) a += ss[i];
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) a += __shfl_xor(a, sh);
    if (p.segments_out)
        for (int i = lane; i < p.NS0; i += 64) p.segments_out[(long long)pb * p.NS0 + i] = i < S ? ss[i] / (float)ST_BANDS : __builtin_nanf("");
    if (lane == 0) {
        const bool bad = p.bad[b] | p.bad[(long long)p.B + pb];
        p.score[pb] = bad ? __builtin_nanf("") : (S > 0 ? a / ((float)ST_BANDS * (float)S) : 1e-5f);
    }
}

}  // namespace ac
