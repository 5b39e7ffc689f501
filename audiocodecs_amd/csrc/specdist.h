// specdist: the STFT and mel spectral distances of a decoded batch against its reference -- the arithmetic of
// downstream/metrics/stft_distance.py:49-69 and mel_distance.py:57-61 at their defaults (16 kHz, n_fft 1024, hop 320, 80 mels) as one
// split16 MFMA GEMM per frame tile with the whole epilogue in registers.  No spectrogram, magnitude or dB array reaches memory: the
// kernel writes one fp32 per (hypothesis, clip, frame) and metric, a small finish kernel means them.
//   * one wave owns 16 frames of one (hypothesis, clip) pair.  The 15 * 320 + 1024 = 5824 samples those frames cover (reflect padding
//     resolved while loading) lie in LDS as split16 planes, both signals of the pair side by side; a frame is the window of 1024
//     halves that starts 320 j into the slab, so the overlapping frames share their samples.
//   * scale: ONE power of two per signal and tile, from the largest finite magnitude of that slab (amax_acc, s16_exponent) -- a quiet
//     passage keeps its relative precision beside a loud one elsewhere in the clip.  The magnitudes that feed the mel product carry a
//     scale per FRAME, from the largest magnitude of the frame's own 1024 samples (maxima of 64-sample chunks, 16 chunks a frame):
//     |X| <= 512 amax, the window sums to 512.
//   * the DFT is computed TRANSPOSED, C[bin][frame] = sum_n (w[n] trig(2 pi bin n / 1024)) x[frame][n]: the basis is the A operand (rows
//     are bins), the frames are the B operand.  A lane (li, kq) then holds, for frame li, bins 4 kq .. 4 kq + 3 of every 16-bin tile --
//     cos and sin of one bin in the same lane and register -- and the magnitudes of a pass (two bin tiles: 32 bins) are, as they
//     stand, the B operand of one k-step of mel^T[mel][frame] = sum_bin fb[bin][mel] |X|[bin][frame] under the k-order
//     (kq, e) <-> bin 16 (e / 4) + 4 kq + e % 4, which the filterbank planes are stored in.  Nothing is exchanged between lanes
//     until the two squared sums of a frame are added over kq at the very end.
//   * pass = 32 bins: 32 k-steps of 32 samples; every basis fragment is loaded once and multiplies the reference and the hypothesis.
//     17 passes cover bins 0 .. 543; the basis columns of bins 513 .. 543 are zero, both signals get p = 0 there and the term vanishes.
//   * per bin: p = re^2 + im^2, dB = 5 log10(max(p, 1e-20)) (= 10 log10(max(|X|, 1e-10))), |X| = sqrt(p); the two logarithms are
//     subtracted before the factor is applied (5 a - 5 b would contract to an fma that favours one side).  The max is written so that
//     a NaN stays a NaN.  Per mel: dB = 10 log10(max(mel, 1e-10)).
//   * both signals of a pair go through the same instructions and (a - b)^2 == (b - a)^2: swapping them returns the same bits, and
//     equal signals give exactly 0.  A wave reads one clip of one hypothesis: its results depend on nothing else in the call.
//   * tables (built once by sd_tables_kernel from fp64 values computed on the host, ac_specdist_source), scale 2^14:
//         basis[17 passes][32 k-steps][2 bin tiles][cos, sin][hi, lo][64 lanes][8 fp16]     lane (i, kq), e: bin 32 pass + 16 tile + i, n = 32 s + 8 kq + e
//         fb   [17 passes][5 mel tiles][hi, lo][64 lanes][8 fp16]                           lane (i, kq), e: mel 16 mt + i, bin 32 pass + 16 (e / 4) + 4 kq + e % 4
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "split16.h"

namespace ac {

constexpr int SD_NFFT = 1024, SD_HOP = 320, SD_BINS = 513, SD_MELS = 80;
constexpr int SD_FT = 16;                                      // frames per tile (one wave)
constexpr int SD_SLAB = (SD_FT - 1) * SD_HOP + SD_NFFT;        // 5824 samples a tile's frames cover
constexpr int SD_CHUNK = 64, SD_CHUNKS = SD_SLAB / SD_CHUNK;   // 91 chunk maxima: frame j covers chunks 5 j .. 5 j + 15
constexpr int SD_PASSES = 17, SD_KS = SD_NFFT / 32, SD_MT = SD_MELS / 16;
constexpr int SD_S = 14;                                       // s16_exponent(bits of 1.0f): basis and filterbank values are at most 1
constexpr int SD_MAX_P = 4;
constexpr int SD_MAX_L = 1 << 24;
constexpr long long SD_BASIS_HALVES = (long long)SD_PASSES * SD_KS * 8 * 512;
constexpr long long SD_FB_HALVES = (long long)SD_PASSES * SD_MT * 2 * 512;
constexpr int SD_SRC_COUNT = SD_NFFT + SD_BINS * SD_MELS;      // fp64 source: cos(2 pi j / 1024) [1024], fb [513][80]
static_assert(SD_SLAB % SD_CHUNK == 0 && SD_HOP % SD_CHUNK == 0 && 5 * (SD_FT - 1) + 16 == SD_CHUNKS, "chunk maxima tile the frames");

struct SdTablesParams {
    const double* src;       // [SD_SRC_COUNT]
    _Float16* basis;
    _Float16* fb;
};

struct SdParams {
    const float* hyp;        // [P][B][L]
    const float* ref;        // [B][L]
    const _Float16* basis;
    const _Float16* fb;
    float* ws_stft;          // [P][B][F]
    float* ws_mel;           // [P][B][F]
    int B, L, F, tiles;
};

struct SdFinishParams {
    const float* ws_stft;
    const float* ws_mel;
    float* stft_out;         // [P][B]
    float* mel_out;          // [P][B]
    float* stft_frames;      // [P][B][F] or null
    float* mel_frames;       // [P][B][F] or null
    int F;
};

// One thread per (fragment, lane) of either table: 8 values, both planes.
__global__ __launch_bounds__(256) void sd_tables_kernel(const SdTablesParams p) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nb = (long long)SD_PASSES * SD_KS * 4 * 64, nf = (long long)SD_PASSES * SD_MT * 64;
    if (t >= nb + nf) return;
    f16x8 hi, lo;
    if (t < nb) {
        const int lane = (int)(t & 63), i = lane & 15, kq = lane >> 4;
        const int qc = (int)(t >> 6) & 3, s = (int)(t >> 8) & 31, pass = (int)(t >> 13);
        const int bin = 32 * pass + 16 * (qc >> 1) + i;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int n = 32 * s + 8 * kq + e;
            const int j = (bin * n) & 1023;
            const double w = 0.5 * (1.0 - p.src[n]);
            const double v = bin < SD_BINS ? w * p.src[(qc & 1) ? ((j + 768) & 1023) : j] : 0.0;      // sin a = cos(a - pi / 2)
            _Float16 h, l;
            s16_split64(v, h, l);
            hi[e] = h;
            lo[e] = l;
        }
        _Float16* o = p.basis + (((long long)(pass * SD_KS + s) * 4 + qc) * 2) * 512 + lane * 8;
        *reinterpret_cast<f16x8*>(o) = hi;
        *reinterpret_cast<f16x8*>(o + 512) = lo;
    } else {
        const long long u = t - nb;
        const int lane = (int)(u & 63), i = lane & 15, kq = lane >> 4;
        const int mt = (int)((u >> 6) % SD_MT), pass = (int)((u >> 6) / SD_MT);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int bin = 32 * pass + 16 * (e >> 2) + 4 * kq + (e & 3);
            const double v = bin < SD_BINS ? p.src[SD_NFFT + bin * SD_MELS + 16 * mt + i] : 0.0;
            _Float16 h, l;
            s16_split64(v, h, l);
            hi[e] = h;
            lo[e] = l;
        }
        _Float16* o = p.fb + ((long long)(pass * SD_MT + mt) * 2) * 512 + lane * 8;
        *reinterpret_cast<f16x8*>(o) = hi;
        *reinterpret_cast<f16x8*>(o + 512) = lo;
    }
}

// sample g of the reflect-padded signal (g = 0 is 512 samples before the first); 0 beyond the padding (only frames past the last read it)
__device__ __forceinline__ float sd_sample(const float* sig, int L, int g) {
    int t = g - SD_NFFT / 2;
    t = t < 0 ? -t : (t >= L ? 2 * (L - 1) - t : t);
    return (t >= 0 && t < L) ? sig[t] : 0.f;
}

// dB with the floor applied so that a NaN stays one (fmaxf would return the floor)
__device__ __forceinline__ float sd_log10_floor(float v, float floor_) { return log10f(v < floor_ ? floor_ : v); }

__global__ __launch_bounds__(64) void specdist_kernel(const SdParams p) {
#pragma clang fp contract(off)      // every fma below is written out: both signals of a pair take the same roundings
    __shared__ __attribute__((aligned(16))) _Float16 planes[2][2][SD_SLAB];      // [signal][hi, lo][sample]
    __shared__ unsigned cmax[2][SD_CHUNKS + 1];
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int tile = (int)(blockIdx.x % (unsigned)p.tiles), b = (int)(blockIdx.x / (unsigned)p.tiles), hp = blockIdx.y;
    const int g0 = tile * SD_FT * SD_HOP;
    const float* sig[2] = {p.ref + (long long)b * p.L, p.hyp + ((long long)hp * p.B + b) * p.L};

    float inv[2];          // 2^-(s + 14): accumulator -> spectrum
    float msc[2], minv[2]; // this lane's frame: magnitude -> operand, mel accumulator -> mel
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        unsigned am = 0;
        for (int c = 0; c < SD_CHUNKS; ++c) {
            unsigned m = 0;
            amax_acc(m, sd_sample(sig[g], p.L, g0 + c * SD_CHUNK + lane));
            m = group_max_u32<64>(m);
            if (lane == 0) cmax[g][c] = m;
            am = m > am ? m : am;
        }
        const int s = s16_exponent(am);
        const float sc = s16_pow2(s);
        inv[g] = s16_pow2(-(s + SD_S));
        for (int c = 0; c < SD_CHUNKS; ++c) {
            const int i = c * SD_CHUNK + lane;
            const float v = sd_sample(sig[g], p.L, g0 + i);
            const _Float16 h = (_Float16)(v * sc);
            planes[g][0][i] = h;
            planes[g][1][i] = (_Float16)__builtin_fmaf(v, sc, -(float)h);
        }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        unsigned fm = 0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const unsigned m = cmax[g][5 * li + c];
            fm = m > fm ? m : fm;
        }
        const int sm = s16_exponent(fm) - 10;            // |X| <= 512 amax:  |X| 2^sm < 2^14
        msc[g] = s16_pow2(sm);
        minv[g] = s16_pow2(-(sm + SD_S));
    }

    float ss = 0.f;
    s16_f32x4 mel[2][SD_MT];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int mt = 0; mt < SD_MT; ++mt) mel[g][mt] = s16_f32x4{0.f, 0.f, 0.f, 0.f};

    const f16x8* bt = reinterpret_cast<const f16x8*>(p.basis) + lane;
    const f16x8* ft = reinterpret_cast<const f16x8*>(p.fb) + lane;
    const int xo = SD_HOP * li + 8 * kq;
    for (int pass = 0; pass < SD_PASSES; ++pass) {
        s16_f32x4 acc[2][4];                             // [signal][tile * 2 + (cos, sin)]
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int qc = 0; qc < 4; ++qc) acc[g][qc] = s16_f32x4{0.f, 0.f, 0.f, 0.f};
        const f16x8* bp = bt + (long long)pass * SD_KS * 8 * 64;
        f16x8 cur[8], nxt[8];
#pragma unroll
        for (int f = 0; f < 8; ++f) cur[f] = bp[f * 64];
#pragma unroll 2
        for (int s = 0; s < SD_KS; ++s) {
            const int sn = s + 1 < SD_KS ? s + 1 : s;    // (the look-ahead past the end re-reads the last k-step)
#pragma unroll
            for (int f = 0; f < 8; ++f) nxt[f] = bp[(sn * 8 + f) * 64];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const f16x8 xh = *reinterpret_cast<const f16x8*>(&planes[g][0][xo + 32 * s]);
                const f16x8 xl = *reinterpret_cast<const f16x8*>(&planes[g][1][xo + 32 * s]);
#pragma unroll
                for (int qc = 0; qc < 4; ++qc) acc[g][qc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[qc * 2], xl, acc[g][qc], 0, 0, 0);
#pragma unroll
                for (int qc = 0; qc < 4; ++qc) acc[g][qc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[qc * 2 + 1], xh, acc[g][qc], 0, 0, 0);
#pragma unroll
                for (int qc = 0; qc < 4; ++qc) acc[g][qc] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur[qc * 2], xh, acc[g][qc], 0, 0, 0);
            }
#pragma unroll
            for (int f = 0; f < 8; ++f) cur[f] = nxt[f];
        }
        // the pass's 8 bins of this lane's frame: dB difference into the running sum, magnitudes into the mel product
        float lg[2][8];
        f16x8 mh[2], ml[2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float re = acc[g][(e >> 2) * 2][e & 3] * inv[g], im = acc[g][(e >> 2) * 2 + 1][e & 3] * inv[g];
                const float pw = __builtin_fmaf(re, re, im * im);
                lg[g][e] = sd_log10_floor(pw, 1e-20f);
                const float mag = sqrtf(pw);
                const _Float16 h = (_Float16)(mag * msc[g]);
                mh[g][e] = h;
                ml[g][e] = (_Float16)__builtin_fmaf(mag, msc[g], -(float)h);
            }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float d = 5.0f * (lg[1][e] - lg[0][e]);      // the difference FIRST: a - b == -(b - a), where 5 a - 5 b may contract to an fma on one side
            ss = __builtin_fmaf(d, d, ss);
        }
        const f16x8* fp = ft + (long long)pass * SD_MT * 2 * 64;
#pragma unroll
        for (int mt = 0; mt < SD_MT; ++mt) {
            const f16x8 fh = fp[(mt * 2) * 64], fl = fp[(mt * 2 + 1) * 64];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                mel[g][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh, ml[g], mel[g][mt], 0, 0, 0);
                mel[g][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fl, mh[g], mel[g][mt], 0, 0, 0);
                mel[g][mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fh, mh[g], mel[g][mt], 0, 0, 0);
            }
        }
    }
    float sm = 0.f;
#pragma unroll
    for (int mt = 0; mt < SD_MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = 10.0f * (sd_log10_floor(mel[1][mt][r] * minv[1], 1e-10f) - sd_log10_floor(mel[0][mt][r] * minv[0], 1e-10f));
            sm = __builtin_fmaf(d, d, sm);
        }
    // the four lanes of a frame (kq = 0 .. 3) hold disjoint bins and mels
    ss += __shfl_xor(ss, 16);
    ss += __shfl_xor(ss, 32);
    sm += __shfl_xor(sm, 16);
    sm += __shfl_xor(sm, 32);
    const int f = tile * SD_FT + li;
    if (kq == 0 && f < p.F) {
        const long long o = ((long long)hp * p.B + b) * p.F + f;
        p.ws_stft[o] = sqrtf(ss);
        p.ws_mel[o] = sqrtf(sm);
    }
}

// One wave per (hypothesis, clip): lane l adds frames l, l + 64, ... in order, the 64 sums fold by an xor butterfly -- an order that
// depends on F alone.
__global__ __launch_bounds__(64) void specdist_finish_kernel(const SdFinishParams p) {
    const int lane = threadIdx.x & 63;
    const long long o = (long long)blockIdx.x * p.F;
    float a = 0.f, m = 0.f;
    for (int f = lane; f < p.F; f += 64) {
        const float x = p.ws_stft[o + f], y = p.ws_mel[o + f];
        a += x;
        m += y;
        if (p.stft_frames) p.stft_frames[o + f] = x;
        if (p.mel_frames) p.mel_frames[o + f] = y;
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        a += __shfl_xor(a, sh);
        m += __shfl_xor(m, sh);
    }
    if (lane == 0) {
        p.stft_out[blockIdx.x] = a / (float)p.F;
        p.mel_out[blockIdx.x] = m / (float)p.F;
    }
}

}  // namespace ac
