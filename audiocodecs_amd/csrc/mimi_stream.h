// Streaming Mimi encode (mimi_stream.hip): the small kernels of one push.  The convs and linear layers of a push are the
// batch path's tap-GEMMs; what is new is the state the stream carries between pushes (DESIGN.md "Streaming Mimi encode"):
//   mstream_stage_kernel   [cache | chunk] -> staged input of one causal conv, and the chunk's last P rows -> cache
//   mstream_rope_kernel    RoPE of the push's q and k rows at each stream's absolute positions
//   mstream_attn_kernel    the push's queries against [ring || new keys] under the sliding-window causal mask
//   mstream_append_kernel  the push's last keys / values -> the ring (a later launch than the attention: ring-overwrite rule)
//   mstream_advance_kernel position += rows, fresh = 0 (the last launch of a push)
//   mstream_reset_kernel   header + (masked) position = 0, fresh = 1; the rings are not touched
// Streaming decode (DESIGN.md "Streaming Mimi decode") adds
//   mstream_stage_ro_kernel + mstream_cache_tail_kernel   the same staging for a chunk SHORTER than the history (L < P), in two launches
//   mstream_upsample_kernel  the depthwise stride-s transposed conv on [previous input row | chunk]
//   mstream_linear_kernel    Y[R][N] = epilogue(X[R][K] W^T) for the few rows of a push: weights streamed, exact fp32 FMAs
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tap_gemm.h"

constexpr unsigned MSTREAM_MAGIC = 0x5453434du;   // "MCST"
constexpr unsigned MDSTREAM_MAGIC = 0x5453444du;  // "MDST": a decode state (its own layout; never accepted where an encode state is expected)
constexpr int MSTREAM_MAXHD = 64;

struct MStreamHeader {           // the first bytes of a state buffer
    unsigned magic, version;
    unsigned long long fingerprint;   // FNV-1a of the handle's ac_mimi_config (device field excluded)
    int B, pad;
};

struct MStreamStageParams {
    float* cache;                // [B][P][C]
    const float* x;              // chunk rows: x + b*bs + t*ts, C contiguous channels
    long long bs, ts;
    float* y;                    // [B][P+L][C]
    const int* fresh;            // [B]
    int B, P, L, C;
    int replicate;               // a fresh stream's history: 0 = zeros, 1 = its first chunk row repeated (pad_mode="replicate")
};

// one thread per (b, staged row, channel).  The thread that reads cache row r is the only one that rewrites it (needs L >= P).
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
            float* cr = p.cache + ((long long)b * p.P + r) * p.C + c;
            v = p.fresh[b] ? (p.replicate ? xb[c] : 0.f) : *cr;
            *cr = xb[(long long)(p.L - p.P + r) * p.ts + c];
        } else {
            v = xb[(long long)(r - p.P) * p.ts + c];
        }
        p.y[e] = v;
    }
}

// The same staging for ANY L >= 1, in two launches.  With L < P a cache row is read by one thread (as history row r) and rewritten
// from another thread's source (the new cache is the last P rows of [cache | chunk], which overlaps the old cache): this kernel only
// reads the cache, and mstream_cache_tail_kernel, a later launch on the same stream, copies the staged buffer's last P rows into it.
__global__ __launch_bounds__(256) void mstream_stage_ro_kernel(const MStreamStageParams p) {
    const long long rows = (long long)p.P + p.L;
    const long long n = (long long)p.B * rows * p.C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % p.C);
        const long long br = e / p.C;
        const int r = (int)(br % rows), b = (int)(br / rows);
        const float* xb = p.x + (long long)b * p.bs;
        float v;
        if (r < p.P) v = p.fresh[b] ? (p.replicate ? xb[c] : 0.f) : p.cache[((long long)b * p.P + r) * p.C + c];
        else v = xb[(long long)(r - p.P) * p.ts + c];
        p.y[e] = v;
    }
}

// staged rows [L, L + P) of every stream -> its cache (p.y is read here)
__global__ __launch_bounds__(256) void mstream_cache_tail_kernel(const MStreamStageParams p) {
    const long long n = (long long)p.B * p.P * p.C;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % p.C);
        const long long br = e / p.C;
        const int r = (int)(br % p.P), b = (int)(br / p.P);
        p.cache[e] = p.y[((long long)b * (p.P + p.L) + p.L + r) * p.C + c];
    }
}

struct MStreamUpsampleParams {
    const float* xs;             // staged [B][N + 1][C]: row 0 = the stream's previous input row (zeros when fresh)
    const float* w;              // [C][2 * s]
    float* y;                    // [B][N * s][C]
    int B, N, C, s;
};

// upsample_dw_kernel (mimi.h) on a staged input: y[i*s + ph][c] = x[i][c] w[c][ph] + x[i-1][c] w[c][ph + s], the same two products and sum
__global__ __launch_bounds__(256) void mstream_upsample_kernel(const MStreamUpsampleParams p) {
    const int c4 = p.C / 4;
    const long long total = (long long)p.B * p.N * p.s * c4;
    for (long long gid = (long long)blockIdx.x * 256 + threadIdx.x; gid < total; gid += (long long)gridDim.x * 256) {
        const int q = (int)(gid % c4);
        const long long row = gid / c4;                         // b*(N*s) + t
        const int t = (int)(row % ((long long)p.N * p.s));
        const long long b = row / ((long long)p.N * p.s);
        const int i = t / p.s, ph = t % p.s, k = 2 * p.s;
        const float* xb = p.xs + b * (p.N + 1) * p.C;
        const ac::f32x4 x0 = *reinterpret_cast<const ac::f32x4*>(xb + (long long)i * p.C + 4 * q);
        const ac::f32x4 x1 = *reinterpret_cast<const ac::f32x4*>(xb + (long long)(i + 1) * p.C + 4 * q);
        ac::f32x4 y;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* wc = p.w + (long long)(4 * q + u) * k;
            y[u] = __fadd_rn(__fmul_rn(x0[u], wc[ph + p.s]), __fmul_rn(x1[u], wc[ph]));
        }
        *reinterpret_cast<ac::f32x4*>(p.y + row * p.C + 4 * q) = y;
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

struct MStreamRopeParams {
    float* qkv;                  // [B][T][3A] (q | k | v), rotated in place (q and k)
    const long long* pos;        // [B] absolute position of row 0
    int B, T, A, HD;
    float inv[MSTREAM_MAXHD / 2];  // inv_freq (fp32), as the batch table's
};

// x cos + rotate_half(x) sin ([HF] mimi :582-599), each factor as the batch table computes it: angle = inv[j] * (float)p in fp32,
// cos / sin rounded once from double; products and sum unfused like attention_kernel's stage_rope.
__global__ __launch_bounds__(256) void mstream_rope_kernel(const MStreamRopeParams p) {
    const int half = p.HD / 2, heads = p.A / p.HD;
    const long long n = (long long)p.B * p.T * 2 * heads * half;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int j = (int)(e % half);
        long long r = e / half;
        const int hh = (int)(r % heads);
        r /= heads;
        const int which = (int)(r % 2);
        const long long row = r / 2;                  // b*T + t
        const int b = (int)(row / p.T), t = (int)(row % p.T);
        const float ang = p.inv[j] * (float)(p.pos[b] + t);
        const float cv = (float)cos((double)ang), sv = (float)sin((double)ang);
        float* x = p.qkv + row * 3 * p.A + (long long)which * p.A + (long long)hh * p.HD;
        const float lo = x[j], hi = x[j + half];
        x[j] = __fadd_rn(__fmul_rn(lo, cv), __fmul_rn(-hi, sv));
        x[j + half] = __fadd_rn(__fmul_rn(hi, cv), __fmul_rn(lo, sv));
    }
}

struct MStreamAttnParams {
    const float* qkv;            // [B][T][3A], q and k rotated
    const float* rk;             // ring of this layer: [B][R][A] keys (rotated) and values; slot = position % R
    const float* rv;
    const long long* pos;        // [B]
    float* out;                  // [B][T][A]
    int B, T, A, HD, window, R;
    float scaling;
};

// One wave per (query row, head, stream), keys 64 at a time (one per lane), online softmax in fp32 with exact FMA products.
// Key j is visible to query i iff j <= i and i - j < window; positions below 0 (before the stream's reset) do not exist.
__global__ __launch_bounds__(256) void mstream_attn_kernel(const MStreamAttnParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int hh = blockIdx.y, b = blockIdx.z;
    if (i >= p.T) return;                                 // (whole wave)
    const long long P0 = p.pos[b], qa = P0 + i;
    const long long rs = 3LL * p.A;
    const float* qrow = p.qkv + ((long long)b * p.T + i) * rs + (long long)hh * p.HD;
    const float qv = lane < p.HD ? qrow[lane] : 0.f;
    long long j0 = qa - p.window + 1;
    if (j0 < 0) j0 = 0;
    float m = -INFINITY, l = 0.f, acc = 0.f;
    auto key_row = [&](long long j, const float* ring, int which) -> const float* {
        if (j >= P0) return p.qkv + ((long long)b * p.T + (j - P0)) * rs + (long long)which * p.A + (long long)hh * p.HD;
        return ring + ((long long)b * p.R + (j % p.R)) * p.A + (long long)hh * p.HD;
    };
    for (long long jb = j0; jb <= qa; jb += 64) {
        const long long j = jb + lane;
        const bool ok = j <= qa;
        float s = 0.f;
        const float* kr = key_row(ok ? j : qa, p.rk, 1);
        for (int d = 0; d < p.HD; ++d) s = fmaf(__shfl(qv, d), kr[d], s);
        s = ok ? s * p.scaling : -INFINITY;
        float bm = s;
        for (int o = 32; o >= 1; o >>= 1) bm = fmaxf(bm, __shfl_xor(bm, o));
        const float mn = fmaxf(m, bm);
        const float corr = expf(m - mn);                  // (m = -inf on the first block: 0)
        const float e = ok ? expf(s - mn) : 0.f;
        float es = e;
        for (int o = 32; o >= 1; o >>= 1) es += __shfl_xor(es, o);
        l = fmaf(l, corr, es);
        acc *= corr;
        const int cnt = (int)((qa - jb + 1) < 64 ? (qa - jb + 1) : 64);
        for (int k = 0; k < cnt; ++k) {
            const float pk = __shfl(e, k);
            const float* vr = key_row(jb + k, p.rv, 2);
            if (lane < p.HD) acc = fmaf(pk, vr[lane], acc);
        }
        m = mn;
    }
    if (lane < p.HD) p.out[((long long)b * p.T + i) * p.A + (long long)hh * p.HD + lane] = acc / l;
}

struct MStreamAppendParams {
    const float* qkv;            // [B][T][3A]
    float* rk;                   // [B][R][A]
    float* rv;
    const long long* pos;
    int B, T, A, R;
};

// the last min(T, R) rows of the push -> ring slots (position % R)
__global__ __launch_bounds__(256) void mstream_append_kernel(const MStreamAppendParams p) {
    const int keep = p.T < p.R ? p.T : p.R;
    const long long n = (long long)p.B * keep * p.A;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % p.A);
        const long long r = e / p.A;
        const int t = p.T - keep + (int)(r % keep), b = (int)(r / keep);
        const float* src = p.qkv + ((long long)b * p.T + t) * 3 * p.A + c;
        long long r_ = (p.pos[b] + t) % p.R;
        if (r_ < 0) r_ += p.R;                        // (a position is never negative once reset; the slot stays in the ring regardless)
        const long long slot = ((long long)b * p.R + r_) * p.A + c;
        p.rk[slot] = src[p.A];
        p.rv[slot] = src[2 * p.A];
    }
}

__global__ __launch_bounds__(64) void mstream_advance_kernel(long long* pos, int* fresh, int B, int rows) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) {
        pos[b] += rows;
        fresh[b] = 0;
    }
}

__global__ __launch_bounds__(64) void mstream_reset_kernel(MStreamHeader* hdr, MStreamHeader h, long long* pos, int* fresh, const uint8_t* mask, int B) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b == 0) *hdr = h;
    if (b < B && (!mask || mask[b])) {
        pos[b] = 0;
        fresh[b] = 1;
    }
}
