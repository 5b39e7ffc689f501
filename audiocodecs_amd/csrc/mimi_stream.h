// Streaming Mimi encode (mimi_stream.hip): the small kernels of one push.  The convs and linear layers of a push are the
// batch path's tap-GEMMs; what is new is the state the stream carries between pushes (DESIGN.md "Streaming Mimi encode"):
//   mstream_rope_kernel    RoPE of the push's q and k rows at each stream's absolute positions
//   mstream_attn_kernel    the push's queries against [ring || new keys] under the sliding-window causal mask
//   mstream_append_kernel  the push's last keys / values -> the ring (a later launch than the attention: ring-overwrite rule)
// Streaming decode (DESIGN.md "Streaming Mimi decode") adds
//   mstream_upsample_kernel  the depthwise stride-s transposed conv on [previous input row | chunk]
// The staging, linear, advance and reset kernels (mstream_stage*_kernel, mstream_cache_tail_kernel, mstream_linear_kernel,
// mstream_advance_kernel, mstream_reset_kernel; a reset does not touch the rings) are shared with the EnCodec stream: stream_stage.h.
// A slot push (ac_mimi_stream_*_slots) runs n listed streams of the `cap` the state holds: qkv and out stay dense
// [n] rows, and only the position and the ring rows go through the slot map (`slot`, stream_stage.h mstream_slot; null = identity,
// the lockstep push, whose code path is untouched).  A row whose entry is outside [0, cap) is at position 0, reads no ring row -- at
// position 0 every visible key lies in the push -- and appends nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tap_gemm.h"
#include "stream_stage.h"

constexpr unsigned MSTREAM_MAGIC = 0x5453434du;   // "MCST"
constexpr unsigned MDSTREAM_MAGIC = 0x5453444du;  // "MDST": a decode state (its own layout; never accepted where an encode state is expected)
constexpr int MSTREAM_MAXHD = 64;

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

struct MStreamRopeParams {
    float* qkv;                  // [B][T][3A] (q | k | v), rotated in place (q and k)
    const long long* pos;        // [B] absolute position of row 0
    int B, T, A, HD;
    float inv[MSTREAM_MAXHD / 2];  // inv_freq (fp32), as the batch table's
    const int* slot = nullptr;   // null: row b is stream b.  Else [B] (device): pos[slot[b]] of the `cap` streams the state holds
    int cap = 0;
};

// the stream of row b in a slot push (-1: none) and its position (0 for none)
__device__ __forceinline__ long long mstream_slot_pos(const long long* pos, const int* slot, int b, int cap, int* sb) {
    *sb = mstream_slot(slot, b, cap);
    return *sb >= 0 ? pos[*sb] : 0;
}

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
        int sb;
        const long long p0 = p.slot ? mstream_slot_pos(p.pos, p.slot, b, p.cap, &sb) : p.pos[b];
        const float ang = p.inv[j] * (float)(p0 + t);
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
    const int* slot = nullptr;   // null: row b is stream b.  Else [B] (device): position and ring rows of stream slot[b] of `cap`
    int cap = 0;
};

// One wave per (query row, head, stream), keys 64 at a time (one per lane), online softmax in fp32 with exact FMA products.
// Key j is visible to query i iff j <= i and i - j < window; positions below 0 (before the stream's reset) do not exist.
// In a slot push every blockIdx.z has its own position: ring phase, window start and number of key blocks are per wave.
__global__ __launch_bounds__(256) void mstream_attn_kernel(const MStreamAttnParams p) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int hh = blockIdx.y, b = blockIdx.z;
    if (i >= p.T) return;                                 // (whole wave)
    int sb = b;                                           // the stream whose ring this row reads
    long long P0;
    if (p.slot) {
        P0 = mstream_slot_pos(p.pos, p.slot, b, p.cap, &sb);
        if (sb < 0) sb = 0;                               // (P0 = 0: no key below it, the ring is not read)
    } else {
        P0 = p.pos[b];
    }
    const long long qa = P0 + i;
    const long long rs = 3LL * p.A;
    const float* qrow = p.qkv + ((long long)b * p.T + i) * rs + (long long)hh * p.HD;
    const float qv = lane < p.HD ? qrow[lane] : 0.f;
    long long j0 = qa - p.window + 1;
    if (j0 < 0) j0 = 0;
    float m = -INFINITY, l = 0.f, acc = 0.f;
    auto key_row = [&](long long j, const float* ring, int which) -> const float* {
        if (j >= P0) return p.qkv + ((long long)b * p.T + (j - P0)) * rs + (long long)which * p.A + (long long)hh * p.HD;
        return ring + ((long long)sb * p.R + (j % p.R)) * p.A + (long long)hh * p.HD;
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
    const int* slot = nullptr;   // null: row b is stream b.  Else [B] (device): position and ring rows of stream slot[b] of `cap`
    int cap = 0;
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
        int sb = b;
        long long p0;
        if (p.slot) {
            p0 = mstream_slot_pos(p.pos, p.slot, b, p.cap, &sb);
            if (sb < 0) continue;                     // (a row of no stream appends nothing)
        } else {
            p0 = p.pos[b];
        }
        long long r_ = (p0 + t) % p.R;
        if (r_ < 0) r_ += p.R;                        // (a position is never negative once reset; the slot stays in the ring regardless)
        const long long slot = ((long long)sb * p.R + r_) * p.A + c;
        p.rk[slot] = src[p.A];
        p.rv[slot] = src[2 * p.A];
    }
}
