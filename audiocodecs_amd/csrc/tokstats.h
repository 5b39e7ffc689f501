// tokstats: the token histogram and the per-codebook utilisation figures of downstream/metrics/codebook_util.py.
//   * tokstats_accumulate: ONE pass over toks [B][N][K] (int64, K fastest) adds into caller-owned state: counts [K][C], the number of
//     frames counted (total) and the number of ids outside [0, C) (bad: not counted, never an index).  Reads are flat: lane l of a wave
//     reads element i + l, the codebook of element i is i % K, its frame i / K.  Frames at n >= nvalid[b] are skipped (nvalid may be null).
//   * two forms, chosen on the host from (K, C) alone (ts_group):
//       tiled   C <= 16384.  A workgroup keeps the uint32 histogram of G = min(K, 64 KB / 4 C) codebooks in LDS, walks a grid-stride range
//               of the elements with LDS atomic adds and flushes its non-zero bins with 64-bit global atomic adds.  With G < K the
//               codebook groups are grid dimension y and every group reads the tokens again (a few MB at most), ignoring what is not its own.
//       direct  16384 < C <= 2^20: one 64-bit global atomic add per token, no LDS.
//   * no wrap: a workgroup meets at most ceil(E / (blocks * 256)) * 256 elements, E = B N K <= 2^40 and blocks = 1024 from E = 2^22 on,
//     so a private bin holds at most 2^30 + 256 < 2^32.
//   * tokstats_summary: one workgroup per codebook; valid bins, entropy in bits, utilisation and normalised entropy in fp64, summed in a
//     fixed order (a thread's bins ascending, 64 lanes by an xor butterfly, four waves in order): the same state gives the same bits.
// Neither launch is sized by anything the device computes; nothing is read back.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ac {

constexpr int TS_MAX_K = 64;
constexpr int TS_MIN_C = 2;
constexpr int TS_MAX_C = 1 << 20;
constexpr int TS_TILED_MAX_C = 16384;
constexpr int TS_LDS_BYTES = 65536;
constexpr int TS_BLOCK = 256;
constexpr int TS_MAX_BLOCKS = 1024;
constexpr long long TS_ELEMS_PER_BLOCK = 4096;
constexpr long long TS_MAX_ELEMS = 1ll << 40;

// codebooks per workgroup of the tiled form; 0 = the direct form.  (K, C) are in range.
__host__ __device__ inline int ts_group(int K, int C) {
    if (C > TS_TILED_MAX_C) return 0;
    const int g = TS_LDS_BYTES / (4 * C);
    return g < K ? g : K;
}

struct TokstatsParams {
    const long long* toks;          // [E]
    const int* nvalid;              // [B] or null
    unsigned long long* counts;     // [K][C]
    unsigned long long* total;
    unsigned long long* bad;
    long long E, N;
    int K, C, G;
};

// whether frame `row` (= b N + n) is counted
template <typename I>
__device__ __forceinline__ bool ts_frame_counts(const TokstatsParams& p, I row) {
    if (!p.nvalid) return true;
    const I b = row / (I)p.N;
    return (long long)(row - b * (I)p.N) < (long long)p.nvalid[b];
}

// a wave's sum of the two per-thread tallies goes out as one atomic each, and only when there is something to add
__device__ __forceinline__ void ts_flush_tallies(const TokstatsParams& p, unsigned long long nframes, unsigned long long nbad) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        nframes += __shfl_xor(nframes, sh);
        nbad += __shfl_xor(nbad, sh);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nframes) atomicAdd(p.total, nframes);
        if (nbad) atomicAdd(p.bad, nbad);
    }
}

// I: the type of the element index (unsigned while E <= 2^31: the stride cannot carry it past 2^32)
template <typename I>
__global__ __launch_bounds__(TS_BLOCK) void tokstats_tiled_kernel(const TokstatsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned ts_hist[];      // [gk][C]
    const int k0 = blockIdx.y * p.G;
    const int gk = p.K - k0 < p.G ? p.K - k0 : p.G;
    const int bins = gk * p.C;
    for (int j = threadIdx.x; j < bins; j += TS_BLOCK) ts_hist[j] = 0u;
    __syncthreads();
    unsigned long long nframes = 0, nbad = 0;
    const I E = (I)p.E, stride = (I)gridDim.x * TS_BLOCK;
    for (I i = (I)blockIdx.x * TS_BLOCK + threadIdx.x; i < E; i += stride) {
        const I row = i / (I)p.K;
        const int kl = (int)(i - row * (I)p.K) - k0;
        if (kl < 0 || kl >= gk) continue;
        if (!ts_frame_counts<I>(p, row)) continue;
        const unsigned long long t = (unsigned long long)p.toks[i];
        if (kl + k0 == 0) ++nframes;
        if (t < (unsigned long long)p.C) atomicAdd(&ts_hist[kl * p.C + (int)t], 1u);
        else ++nbad;
    }
    __syncthreads();
    unsigned long long* out = p.counts + (size_t)k0 * p.C;
    for (int j = threadIdx.x; j < bins; j += TS_BLOCK) {
        const unsigned v = ts_hist[j];
        if (v) atomicAdd(out + j, (unsigned long long)v);
    }
    ts_flush_tallies(p, nframes, nbad);
}

template <typename I>
__global__ __launch_bounds__(TS_BLOCK) void tokstats_direct_kernel(const TokstatsParams p) {
    unsigned long long nframes = 0, nbad = 0;
    const I E = (I)p.E, stride = (I)gridDim.x * TS_BLOCK;
    for (I i = (I)blockIdx.x * TS_BLOCK + threadIdx.x; i < E; i += stride) {
        const I row = i / (I)p.K;
        const int k = (int)(i - row * (I)p.K);
        if (!ts_frame_counts<I>(p, row)) continue;
        const unsigned long long t = (unsigned long long)p.toks[i];
        if (k == 0) ++nframes;
        if (t < (unsigned long long)p.C) atomicAdd(p.counts + (size_t)k * p.C + (size_t)t, 1ull);
        else ++nbad;
    }
    ts_flush_tallies(p, nframes, nbad);
}

// out [K][4] = (valid bins, entropy in bits, utilisation, normalised entropy)
__global__ __launch_bounds__(TS_BLOCK) void tokstats_summary_kernel(const unsigned long long* counts, const unsigned long long* total, int C,
                                                                    double* out) {
    __shared__ double sh_h[TS_BLOCK / 64];
    __shared__ unsigned sh_v[TS_BLOCK / 64];
    const unsigned long long tot = *total;
    const unsigned long long* row = counts + (size_t)blockIdx.x * C;
    const double dt = (double)tot;
    double h = 0.0;
    unsigned v = 0;
    if (tot)
        for (int c = threadIdx.x; c < C; c += TS_BLOCK) {
            const unsigned long long n = row[c];
            if (n) {
                const double pr = (double)n / dt;
                h -= pr * log2(pr);
                ++v;
            }
        }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        h += __shfl_xor(h, sh);
        v += __shfl_xor(v, sh);
    }
    if ((threadIdx.x & 63) == 0) {
        sh_h[threadIdx.x >> 6] = h;
        sh_v[threadIdx.x >> 6] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double H = 0.0;
        unsigned valid = 0;
        for (int w = 0; w < TS_BLOCK / 64; ++w) {
            H += sh_h[w];
            valid += sh_v[w];
        }
        const bool many = valid > 1;
        double* o = out + (size_t)blockIdx.x * 4;
        o[0] = (double)valid;
        o[1] = H;
        o[2] = many ? (double)valid / (double)C : 0.0;
        o[3] = many ? H / log2((double)valid) : 0.0;
    }
}

}  // namespace ac
