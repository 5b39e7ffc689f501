// What the streaming paths of the codecs share (mimi_stream.hip, encodec_stream.hip): the state a stream carries between pushes and the
// small kernels that move it.
//   mstream_stage_kernel   [cache | chunk] -> staged input of one causal conv, and the chunk's last P rows -> cache
//   mstream_stage_ro_kernel + mstream_cache_tail_kernel   the same staging for a chunk SHORTER than the history (L < P), in two launches
//   mstream_linear_kernel  Y[R][N] = epilogue(X[R][K] W^T) for the few rows of a push: weights streamed, exact fp32 FMAs
//   mstream_advance_kernel position += rows, fresh = 0 (the last launch of a push)
//   mstream_reset_kernel   header + (masked) position = 0, fresh = 1
// A push may serve a SUBSET of the state's streams: its activations are dense ([n] rows), and only the addresses into the stream state
// (cache, fresh, position) go through a slot map -- `slot` [n], row b of the push belongs to stream slot[b]; null = identity
// (mstream_slot).  Lockstep pushes pass null; the slot pushes of both codecs pass the caller's list (encodec_stream.hip, mimi_stream.hip).
// Every kernel here is a template (the dummy parameter of those that need none): two translation units include this header, and the
// library keeps one definition of every non-template kernel (core.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tap_gemm.h"

struct MStreamHeader {           // the first bytes of a state buffer
    unsigned magic, version;
    unsigned long long fingerprint;   // FNV-1a of the handle's configuration struct (device field excluded)
    int B, pad;
};

// a fresh stream's history (MStreamStageParams::replicate): what the codec's padding puts left of the clip's first row
constexpr int STAGE_ZERO = 0;        // zeros (pad_mode="constant": Mimi; every transposed conv)
constexpr int STAGE_REPLICATE = 1;   // the first chunk row repeated (pad_mode="replicate": Mimi's down-sampler)
constexpr int STAGE_REFLECT = 2;     // history row -i = chunk row i (pad_mode="reflect": EnCodec); the first chunk must be longer than P

struct MStreamStageParams {
    float* cache;                // [B][P][C]
    const float* x;              // chunk rows: x + b*bs + t*ts, C contiguous channels
    long long bs, ts;
    float* y;                    // [B][P+L][C]
    const int* fresh;            // [B]
    int B, P, L, C;
    int replicate;               // a fresh stream's history: STAGE_*
    const int* slot;             // null: row b is stream b.  Else [B] (device): row b is stream slot[b] of the `cap` the state holds
    int cap;
};

// The stream of the state that row b of a push addresses, or -1 when the map's entry is outside [0, cap): such a row neither reads nor
// writes the state, whatever the device copy of the list holds.
__device__ __forceinline__ int mstream_slot(const int* slot, int b, int cap) {
    if (!slot) return b;
    const int s = slot[b];
    return (unsigned)s < (unsigned)cap ? s : -1;
}

// history row r (0 .. P-1, position r - P) of a fresh stream
__device__ __forceinline__ float mstream_fresh_row(const MStreamStageParams& p, const float* xb, int r, int c) {
    if (p.replicate == STAGE_REFLECT) return xb[(long long)(p.P - r) * p.ts + c];
    return p.replicate ? xb[c] : 0.f;
}

// one thread per (b, staged row, channel).  The thread that reads cache row r is the only one that rewrites it (needs L >= P).
template <int U = 0>
__global__ __launch_bounds__(256) void mstream_stage_kernel(const MStreamStageParams p) {
    const long long rows = (long long)p.P + p.L;
    const long long n = (long long)p.B * rows * p.C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % p.C);
        const long long br = e / p.C;
        const int r = (int)(br % rows), b = (int)(br / rows);
        const float* xb = p.x + (long long)b * p.bs;
        float v;
        if (r < p.P) {
            const int sb = mstream_slot(p.slot, b, p.cap);
            v = 0.f;
            if (sb >= 0) {
                float* cr = p.cache + ((long long)sb * p.P + r) * p.C + c;
                v = p.fresh[sb] ? mstream_fresh_row(p, xb, r, c) : *cr;
                *cr = xb[(long long)(p.L - p.P + r) * p.ts + c];
            }
        } else {
            v = xb[(long long)(r - p.P) * p.ts + c];
        }
        p.y[e] = v;
    }
}

// The same staging for ANY L >= 1, in two launches.  With L < P a cache row is read by one thread (as history row r) and rewritten
// from another thread's source (the new cache is the last P rows of [cache | chunk], which overlaps the old cache): this kernel only
// reads the cache, and mstream_cache_tail_kernel, a later launch on the same stream, copies the staged buffer's last P rows into it.
template <int U = 0>
__global__ __launch_bounds__(256) void mstream_stage_ro_kernel(const MStreamStageParams p) {
    const long long rows = (long long)p.P + p.L;
    const long long n = (long long)p.B * rows * p.C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % p.C);
        const long long br = e / p.C;
        const int r = (int)(br % rows), b = (int)(br / rows);
        const float* xb = p.x + (long long)b * p.bs;
        float v;
        if (r < p.P) {
            const int sb = mstream_slot(p.slot, b, p.cap);
            v = 0.f;
            if (sb >= 0) v = p.fresh[sb] ? mstream_fresh_row(p, xb, r, c) : p.cache[((long long)sb * p.P + r) * p.C + c];
        } else {
            v = xb[(long long)(r - p.P) * p.ts + c];
        }
        p.y[e] = v;
    }
}

// staged rows [L, L + P) of every stream -> its cache (p.y is read here)
template <int U = 0>
__global__ __launch_bounds__(256) void mstream_cache_tail_kernel(const MStreamStageParams p) {
    const long long n = (long long)p.B * p.P * p.C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % p.C);
        const long long br = e / p.C;
        const int r = (int)(br % p.P), b = (int)(br / p.P);
        const int sb = mstream_slot(p.slot, b, p.cap);
        if (sb >= 0) p.cache[((long long)sb * p.P + r) * p.C + c] = p.y[((long long)b * (p.P + p.L) + p.L + r) * p.C + c];
    }
}

// ---------------------------------------------------------------------------------------------
// The skinny linear layer of a push.  A one-frame push multiplies 2 B rows by the transformer's [N][K] matrices; on a 256-row
// MFMA tile that is one live row pair per tile and the launch costs what 256 rows would.  Here the weights are the only traffic:
//   grid (N, ceil(R / RB)); a workgroup owns ONE output column n and RB rows; its KS waves split the column's K weights into KS
//   contiguous parts; a lane reads 16 bytes of the weight row per step (a wave-instruction covers 1 KiB of it), the same columns of
//   the RB activation rows (a few KB shared by every workgroup: L2), and keeps RB fp32 accumulators.
// Summation order of an output element: lane l of part q adds, in ascending k, the products at k = q K/KS + 4 l + 256 i + (0..3) with
// one fmaf each; the 64 lanes fold by the xor butterfly 32, 16, .. 1; the parts add in the order 0 .. KS-1.  KS is a function of K
// alone (mstream_linear_ks), so the order depends on K only -- not on R, RB, the row's index or the grid: a row's result is
// bit-identical whatever shares the launch.  No atomics, no scratch; exact fp32 products.
// Epilogue as tap_gemm.h epilogue1: GELU, then scale[n] * v, then res + v (res may alias y: the element is read and written by one lane).
// ---------------------------------------------------------------------------------------------
struct MStreamLinearParams {
    const float* x;              // [R][x_pitch], K contiguous floats per row, 16-byte aligned rows
    const float* w;              // [N][K] fp32, row-major (PackedGemm::w_off)
    float* y;                    // [R][y_pitch]
    const float* scale;          // optional [N]
    const float* res;            // optional [R][res_pitch]
    int x_pitch, y_pitch, res_pitch;
    int R, N, K, gelu;
};

constexpr int mstream_linear_ks(int K) { return K >= 1024 && K % 16 == 0 ? 4 : 1; }

template <int RB, int KS>
__global__ __launch_bounds__(64 * KS) void mstream_linear_kernel(const MStreamLinearParams p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x, r0 = blockIdx.y * RB;
    const int kq = p.K / KS;
    const float* wr = p.w + (long long)n * p.K + (long long)wave * kq;
    const float* xr[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int row = r0 + r < p.R ? r0 + r : p.R - 1;          // rows past the end repeat the last one; their sums are not stored
        xr[r] = p.x + (long long)row * p.x_pitch + (long long)wave * kq;
    }
    float acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.f;
#pragma unroll 2
    for (int k = 4 * lane; k < kq; k += 256) {
        const ac::f32x4 wv = *reinterpret_cast<const ac::f32x4*>(wr + k);
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const ac::f32x4 xv = *reinterpret_cast<const ac::f32x4*>(xr[r] + k);
            acc[r] = fmaf(wv.x, xv.x, acc[r]);
            acc[r] = fmaf(wv.y, xv.y, acc[r]);
            acc[r] = fmaf(wv.z, xv.z, acc[r]);
            acc[r] = fmaf(wv.w, xv.w, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc[r] = __fadd_rn(acc[r], __shfl_xor(acc[r], o));
    float v = 0.f;                                                // lane r keeps row r0 + r
#pragma unroll
    for (int r = 0; r < RB; ++r)
        if (lane == r) v = acc[r];
    if constexpr (KS > 1) {
        __shared__ float part[KS][RB];
        if (lane < RB) part[wave][lane] = v;
        __syncthreads();
        if (wave == 0 && lane < RB) {
            v = part[0][lane];
#pragma unroll
            for (int q = 1; q < KS; ++q) v = __fadd_rn(v, part[q][lane]);
        }
    }
    const int row = r0 + lane;
    if (wave == 0 && lane < RB && row < p.R) {
        if (p.gelu) v = ac::gelu1(v);
        if (p.scale) v = __fmul_rn(p.scale[n], v);
        if (p.res) v = __fadd_rn(p.res[(long long)row * p.res_pitch + n], v);
        p.y[(long long)row * p.y_pitch + n] = v;
    }
}

template <int U = 0>
__global__ __launch_bounds__(64) void mstream_advance_kernel(long long* pos, int* fresh, int B, int rows, const int* slot, int cap) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) {
        const int sb = mstream_slot(slot, b, cap);
        if (sb >= 0) {
            pos[sb] += rows;
            fresh[sb] = 0;
        }
    }
}

template <int U = 0>
__global__ __launch_bounds__(64) void mstream_reset_kernel(MStreamHeader* hdr, MStreamHeader h, long long* pos, int* fresh, const uint8_t* mask, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b == 0) *hdr = h;
    if (b < B && (!mask || mask[b])) {
        pos[b] = 0;
        fresh[b] = 1;
    }
}
