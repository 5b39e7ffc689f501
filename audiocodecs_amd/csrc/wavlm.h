// Kernels only the WavLM x-vector speaker encoder needs ([HF] = transformers models/wavlm/modeling_wavlm.py, the model behind the
// reference's SpkSimWavLM, downstream/metrics/speaker_similarity.py:72-123):
//   spk_lens_kernel          per clip: frames that are speech (key limit, rows kept behind the projection) and pooled rows, on the device
//   spk_stem_stats_kernel    Conv1d(1 -> C, k10, s5) recomputed per chunk of frames: per-(clip, channel) partial mean / M2        ([HF]:723-744)
//   spk_stem_norm_kernel     the chunks' moments merged in a fixed order (Chan): mean, 1 / sqrt(var + eps) per (clip, channel)
//   spk_stem_apply_kernel    the conv recomputed, GroupNorm (one group per channel: moments over time), GELU, written once
//   spk_mask_rows_kernel     rows t >= Lf of the projected features to zero                                                   ([HF]:399-402)
//   spk_posconv16_kernel     grouped Conv1d(H, H, k, pad k/2, groups) + bias + GELU + residual, one split16 MFMA GEMM per group ([HF]:48-90)
//   spk_gate_kernel          the gate of the relative-position bias per (clip, head, query)                                   ([HF]:165-176)
//   wavlm_attn16_kernel      softmax(q k^T / 8 + gate * E[bucket(k - q)] | keys < Lf) v, attention16_kernel's scheme (mimi.h)
//   spk_axpy_kernel          acc (+)= w * x: the weighted layer sum as the hidden states appear                               ([HF]:1591-1595)
//   spk_relu_kernel          the TDNN layers' ReLU                                                                            ([HF]:1497)
//   spk_pool_kernel          mean | unbiased std over a clip's own pooled rows                                                ([HF]:1604-1618)
//   spk_cosine_kernel        cosine of embedding pairs, one wave per pair
// The convs 2..7, every Linear, the projector and the TDNN layers run through the tap-GEMM (tap_gemm.h), LayerNorm through layernorm_kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "split16.h"
#include "tap_gemm.h"

namespace ac {

constexpr int SPK_STEM_K = 10, SPK_STEM_S = 5;    // the stem conv (refused otherwise)
constexpr int SPK_STEM_FT = 128;                  // frames per workgroup of the stem kernels

// ---------------------------------------------------------------------------------------------
// lengths.  lens[2 b] = Lf clamped to [1, T]: keys < Lf are visible, rows >= Lf are zeroed; lens[2 b + 1] = pooled rows (may be <= 0)
// ---------------------------------------------------------------------------------------------
__global__ void spk_lens_kernel(const int* __restrict__ valid, int B, long long L, int T, int tdnn_shrink, int* __restrict__ lens) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int Lf = T, np = T - tdnn_shrink;
    if (valid) {
        const long long v = valid[b];
        const long long f = v < 400 ? 0 : (v - 400) / 320 + 1;
        Lf = (int)(f > T ? T : f);
        np = Lf - 8 < T - tdnn_shrink ? Lf - 8 : T - tdnn_shrink;      // the backend's length formula ignores the dilations ([HF]:1541-1554)
    }
    lens[2 * b] = Lf < 1 ? 1 : Lf;
    lens[2 * b + 1] = np;
}

// ---------------------------------------------------------------------------------------------
// Stem.  sig [B][L] -> y [B][T0][C], T0 = (L - 10) / 5 + 1.  The pre-norm conv is never stored: 10 FMAs per value are recomputed
// in each of the three passes over the signal (4 bytes per 5 frames-worth of C outputs: the write of y is the only real traffic).
// ---------------------------------------------------------------------------------------------
struct SpkStemParams {
    const float* sig;    // [B][L]
    const float* w;      // [C][10]
    const float* gn_w;   // [C]
    const float* gn_b;   // [C]
    float* part;         // [B][nch][C][2]: chunk mean, chunk M2
    float* mr;           // [B][C][2]: mean, rstd
    float* y;            // [B][T0][C]
    unsigned* amax;      // optional slot of y (split16.h)
    long long L;
    int T0, C, nch;
    float eps;
};

__device__ __forceinline__ void spk_stem_stage(const SpkStemParams& p, float* s_sig, int b, int f0, int nf) {
    const int n = nf * SPK_STEM_S + (SPK_STEM_K - SPK_STEM_S);
    const float* src = p.sig + (long long)b * p.L + (long long)f0 * SPK_STEM_S;
    for (int i = threadIdx.x; i < n; i += 256) s_sig[i] = src[i];      // (f0 + nf <= T0: the last index is 5 (T0 - 1) + 9 <= L - 1)
    __syncthreads();
}

__global__ __launch_bounds__(256) void spk_stem_stats_kernel(const SpkStemParams p) {
    __shared__ float s_sig[SPK_STEM_FT * SPK_STEM_S + SPK_STEM_K];
    const int b = blockIdx.y, ch = blockIdx.x, f0 = ch * SPK_STEM_FT;
    const int nf = min(SPK_STEM_FT, p.T0 - f0);
    spk_stem_stage(p, s_sig, b, f0, nf);
    for (int c = threadIdx.x; c < p.C; c += 256) {
        float w[SPK_STEM_K];
#pragma unroll
        for (int j = 0; j < SPK_STEM_K; ++j) w[j] = p.w[c * SPK_STEM_K + j];
        float sum = 0.f;
        for (int f = 0; f < nf; ++f) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < SPK_STEM_K; ++j) v = fmaf(w[j], s_sig[f * SPK_STEM_S + j], v);
            sum += v;
        }
        const float mean = sum / (float)nf;
        float m2 = 0.f;
        for (int f = 0; f < nf; ++f) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < SPK_STEM_K; ++j) v = fmaf(w[j], s_sig[f * SPK_STEM_S + j], v);
            const float d = v - mean;
            m2 = fmaf(d, d, m2);
        }
        float* o = p.part + (((long long)b * p.nch + ch) * p.C + c) * 2;
        o[0] = mean;
        o[1] = m2;
    }
}

// one thread per (clip, channel): the chunks in ascending order (the same order whatever the batch or its chunking)
__global__ __launch_bounds__(256) void spk_stem_norm_kernel(const SpkStemParams p) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= p.C) return;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int ch = 0; ch < p.nch; ++ch) {
        const float* q = p.part + (((long long)b * p.nch + ch) * p.C + c) * 2;
        const float nb = (float)min(SPK_STEM_FT, p.T0 - ch * SPK_STEM_FT);
        const float d = q[0] - mean, nn = n + nb;
        mean += d * (nb / nn);
        m2 += q[1] + d * d * (n * nb / nn);
        n = nn;
    }
    float* o = p.mr + ((long long)b * p.C + c) * 2;
    o[0] = mean;
    o[1] = 1.0f / sqrtf(m2 / n + p.eps);       // biased variance (nn.GroupNorm)
}

// thread = (frame lane, 4 channels): 256 / (C / 4) frames side by side, 16-byte stores
__global__ __launch_bounds__(256) void spk_stem_apply_kernel(const SpkStemParams p) {
    __shared__ float s_sig[SPK_STEM_FT * SPK_STEM_S + SPK_STEM_K];
    const int b = blockIdx.y, f0 = blockIdx.x * SPK_STEM_FT;
    const int nf = min(SPK_STEM_FT, p.T0 - f0);
    spk_stem_stage(p, s_sig, b, f0, nf);
    const int nq = p.C / 4, fpb = 256 / nq;
    const int cq = threadIdx.x % nq, fl = threadIdx.x / nq;
    float w[4][SPK_STEM_K], mean[4], sc[4], sh[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = 4 * cq + u;
#pragma unroll
        for (int j = 0; j < SPK_STEM_K; ++j) w[u][j] = p.w[c * SPK_STEM_K + j];
        const float* q = p.mr + ((long long)b * p.C + c) * 2;
        mean[u] = q[0];
        sc[u] = q[1];
        sh[u] = p.gn_b[c];
    }
    const f32x4 gw = *reinterpret_cast<const f32x4*>(p.gn_w + 4 * cq);
    unsigned mx = 0;
    for (int f = fl; f < nf; f += fpb) {
        f32x4 o;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = 0.f;
#pragma unroll
            for (int j = 0; j < SPK_STEM_K; ++j) v = fmaf(w[u][j], s_sig[f * SPK_STEM_S + j], v);
            o[u] = gelu1(fmaf((v - mean[u]) * sc[u], gw[u], sh[u]));      // (x - mean) * rstd * weight + bias, as nn.GroupNorm states it
        }
        amax_acc4(mx, o);
        *reinterpret_cast<f32x4*>(p.y + ((long long)b * p.T0 + f0 + f) * p.C + 4 * cq) = o;
    }
    if (p.amax) amax_flush(mx, amax_at(p.amax, b));
}

// ---------------------------------------------------------------------------------------------
// rows t >= Lf of x [B][T][H] to zero ([HF]:399-402: the zeroed rows ARE the residual and the positional conv's input)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_mask_rows_kernel(float* __restrict__ x, const int* __restrict__ lens, int T, int H4) {
    const int b = blockIdx.y;
    const int Lf = lens[2 * b];
    const long long n = (long long)(T - Lf) * H4;
    f32x4* xb = reinterpret_cast<f32x4*>(x) + ((long long)b * T + Lf) * H4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) xb[i] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------------------------
// Grouped positional conv.  y[b][t][n] = x[b][t][n] + GELU(bias[n] + sum_{j < K} sum_{ci < CG} x[b][t + j - K/2][g CG + ci] w[n][ci][j]),
// n in group g = n / CG, t in [0, T) (the last row of the even-K conv's T + 1 is the one [HF]:37-45 drops).
// One workgroup = 128 output rows of one (clip, group): the group's CG input columns of the rows t0 - K/2 .. t0 + 127 + K/2 - 1 go to LDS
// as fp16 hi / lo planes WITHOUT a row pitch, so that with the contraction index flattened as kf = j CG + ci
//     A[t][kf] = slab[(t + j) CG + ci] = slab[t CG + kf]
// -- an output row's whole contraction is one contiguous run of the slab, and a lane's 8 values of a k-step are one 16-byte read
// whatever CG is (48 is no multiple of the 32-wide step; the order inside a dot product is free as long as both operands share
// it: rvq16.h).  The weights are a Packer::frag16 image of [H][K CG] (kf order), read from L2 straight into the B fragments.
// Arithmetic: split16.h, one power-of-two scale per slab (its largest magnitude: a workgroup reduction), 3 products per step.
// Per wave 32 rows x CG columns: 2 x CG/16 accumulators.
// ---------------------------------------------------------------------------------------------
struct SpkPosConvParams {
    const float* x;          // [B][T][H]
    const _Float16* wimg;    // [H / 16][K CG / 32][2][64][8]
    const float* winv;       // [H]
    const float* bias;       // [H]
    float* y;                // [B][T][H]
    int T, H;
};

template <int CG, int K>
struct SpkPosCfg {
    static constexpr int BM = 128, R = BM + K - 1, NTL = CG / 16, STEPS = K * CG / 32;
    static constexpr int PLANE = R * CG + 8;                         // halfs per plane (+ 8: keeps the second plane 16-byte aligned)
    static constexpr size_t lds_bytes = (size_t)2 * PLANE * 2 + 16;
    static_assert(CG % 16 == 0 && (K * CG) % 32 == 0 && (R * CG) % 8 == 0, "positional conv shape");
};

template <int CG, int K>
__global__ __launch_bounds__(256) void spk_posconv16_kernel(const SpkPosConvParams p) {
    using Cfg = SpkPosCfg<CG, K>;
    constexpr int R = Cfg::R, NTL = Cfg::NTL, STEPS = Cfg::STEPS, PLANE = Cfg::PLANE, Q = CG / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* slab = reinterpret_cast<_Float16*>(smem);
    unsigned* s_mx = reinterpret_cast<unsigned*>(slab + 2 * PLANE);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const int t0 = blockIdx.x * Cfg::BM, g = blockIdx.y, b = blockIdx.z;
    const float* xb = p.x + (long long)b * p.T * p.H + g * CG;
    if (tid == 0) *s_mx = 0u;
    __syncthreads();
    // ---- the slab's largest magnitude
    unsigned mx = 0;
    for (int e = tid; e < R * Q; e += 256) {
        const int row = e / Q, q = e % Q, t = t0 - K / 2 + row;
        if (t >= 0 && t < p.T) amax_acc4(mx, *reinterpret_cast<const f32x4*>(xb + (long long)t * p.H + 4 * q));
    }
    mx = group_max_u32<64>(mx);
    if (lane == 0) atomicMax(s_mx, mx);
    __syncthreads();
    const int ex = s16_exponent(*s_mx);
    const float sx = s16_pow2(ex);
    for (int e = tid; e < R * Q; e += 256) {
        const int row = e / Q, q = e % Q, t = t0 - K / 2 + row;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < p.T) v = *reinterpret_cast<const f32x4*>(xb + (long long)t * p.H + 4 * q);
        split16_store4s(v, sx, slab, PLANE, row * CG + 4 * q);
    }
    __syncthreads();
    f32x4 acc[2][NTL];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) acc[rt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const _Float16* wg = p.wimg + (size_t)g * NTL * STEPS * 1024 + (size_t)lane * 8;
    const _Float16* a0 = slab + (wave * 32 + li) * CG + 8 * kq;
    for (int s = 0; s < STEPS; ++s) {
        f16x8 ah[2], al[2];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt) {
            ah[rt] = *reinterpret_cast<const f16x8*>(a0 + rt * 16 * CG + 32 * s);
            al[rt] = *reinterpret_cast<const f16x8*>(a0 + PLANE + rt * 16 * CG + 32 * s);
        }
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt) {
            const _Float16* wp = wg + ((size_t)nt * STEPS + s) * 1024;
            const f16x8 bh = *reinterpret_cast<const f16x8*>(wp);
            const f16x8 bl = *reinterpret_cast<const f16x8*>(wp + 512);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[rt], bh, acc[rt][nt], 0, 0, 0);
                acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], bl, acc[rt][nt], 0, 0, 0);
                acc[rt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[rt], bh, acc[rt][nt], 0, 0, 0);
            }
        }
    }
    // ---- epilogue: accumulator register r <-> row 4 kq + r, column li
    const float ix = s16_pow2(-ex);
#pragma unroll
    for (int nt = 0; nt < NTL; ++nt) {
        const int n = g * CG + nt * 16 + li;
        const float sc = ix * p.winv[n], bv = p.bias[n];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = t0 + wave * 32 + rt * 16 + 4 * kq + r;
                if (t < p.T) {
                    const long long o = ((long long)b * p.T + t) * p.H + n;
                    p.y[o] = __fadd_rn(p.x[o], gelu1(fmaf(acc[rt][nt][r], sc, bv)));
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------
// Gate of the relative-position bias ([HF]:165-176): x the layer's INPUT, p = Wg x_{q,h} + bg (8 values),
// a = sigmoid(p0 + .. + p3), c = sigmoid(p4 + .. + p7), gate = a (c const_h - 1) + 2.  One thread per (clip, query, head).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_gate_kernel(const float* __restrict__ x, const float* __restrict__ wg, const float* __restrict__ bg,
                                                       const float* __restrict__ cst, float* __restrict__ gate, int B, int T, int heads) {
    __shared__ float s_w[8 * 64 + 8];
    for (int i = threadIdx.x; i < 8 * 64 + 8; i += 256) s_w[i] = i < 512 ? wg[i] : bg[i - 512];
    __syncthreads();
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)B * T * heads) return;
    const int h = (int)(gid % heads);
    const long long bt = gid / heads;
    const float* xr = x + bt * heads * 64 + h * 64;
    f32x4 xv[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) xv[d] = *reinterpret_cast<const f32x4*>(xr + 4 * d);
    float sa = 0.f, sb = 0.f;
#pragma unroll 1
    for (int o = 0; o < 8; ++o) {                              // (the weights are broadcast reads of LDS: every lane the same address)
        float pr = 0.f;
#pragma unroll
        for (int d = 0; d < 16; ++d)
#pragma unroll
            for (int u = 0; u < 4; ++u) pr = fmaf(xv[d][u], s_w[o * 64 + 4 * d + u], pr);
        pr += s_w[512 + o];
        if (o < 4) sa += pr;
        else sb += pr;
    }
    const float ga = 1.0f / (1.0f + __expf(-sa)), gb = 1.0f / (1.0f + __expf(-sb));
    const int t = (int)(bt % T);
    const long long b = bt / T;
    gate[(b * heads + h) * T + t] = fmaf(ga, fmaf(gb, cst[h], -1.0f), 2.0f);
}

// ---------------------------------------------------------------------------------------------
// wavlm_attn16_kernel: attention16_kernel's scheme (mimi.h: transposed products, one query per lane, split16 on
// v_mfma_f32_16x16x32_f16, online softmax, no score tile in memory) for WavLM's attention: bidirectional, no RoPE, no window;
//   score[q][k] = (q . k) / 8 + gate[q] * E[bucket(k - q)][h],   keys k >= Lf masked
// The bias comes from a per-head table of E[bucket(delta)] over delta in [-R, R] (constant beyond: the buckets clamp), of which the
// workgroup keeps the T + 63 entries its 64 queries can meet in LDS; neither the [T][T] bias nor the scores ever exist in HBM.
// Query rows at and beyond Lf are computed like any other (the TDNN's receptive field reaches them: DESIGN.md section 8p).
// Grid (ceil(T / 64), heads, clips); 4 waves, each owns 16 queries.
// ---------------------------------------------------------------------------------------------
struct WavlmAttnParams {
    const float* qkv;     // [B][T][3 A]: q | k | v, head h at columns 64 h
    float* out;           // [B][T][A]
    const float* gate;    // [B][heads][T]
    const float* bias;    // [heads][2 R + 1]
    const int* lens;      // [B][2]: lens[2 b] = visible keys
    int B, T, A, R;
    float scaling;
};

struct WavlmAttnCfg {
    static constexpr int QT = 64, KT = 64, HD = 64, KP = 72;
    static constexpr int PLANE = 64 * KP;
    static constexpr size_t base_bytes = (size_t)4 * PLANE * 2 + 32;
    static size_t lds_bytes(int T) { return base_bytes + (size_t)(T + 64) * 4; }
};

__device__ __forceinline__ void wl_pack8(const f32x4 a, const f32x4 b, const float sc, f16x8& hi, f16x8& lo) {
    const f32x4 s0 = a * sc, s1 = b * sc;
    const f16x4_t h0 = __builtin_convertvector(s0, f16x4_t), h1 = __builtin_convertvector(s1, f16x4_t);
    const f16x4_t l0 = __builtin_convertvector(s0 - __builtin_convertvector(h0, f32x4), f16x4_t);
    const f16x4_t l1 = __builtin_convertvector(s1 - __builtin_convertvector(h1, f32x4), f16x4_t);
    hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

__global__ __launch_bounds__(256, 2) void wavlm_attn16_kernel(const WavlmAttnParams p) {
    using Cfg = WavlmAttnCfg;
    constexpr int KT = Cfg::KT, HD = Cfg::HD, KP = Cfg::KP, PLANE = Cfg::PLANE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* Kp = reinterpret_cast<_Float16*>(smem);         // [2 planes][64 keys][KP]
    _Float16* Vp = Kp + 2 * PLANE;                             // [2 planes][64 dims][KP]  (keys along the row)
    unsigned* slot = reinterpret_cast<unsigned*>(Vp + 2 * PLANE);   // [3 rotating][K, V]
    float* tab = reinterpret_cast<float*>(slot + 8);           // [T + 63]: E[bucket(delta)][h], delta = index - (q0 + 63)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * Cfg::QT, h = blockIdx.y, b = blockIdx.z;
    const long long rs = 3LL * p.A;
    const float* base = p.qkv + (long long)b * p.T * rs + (long long)h * HD;
    const int klim = min(p.lens[2 * b], p.T);
    if (tid < 6) slot[tid] = 0u;
    {
        const float* bh = p.bias + (long long)h * (2 * p.R + 1);
        for (int i = tid; i < p.T + 63; i += 256) {
            const int d = i - (q0 + 63) + p.R;
            tab[i] = bh[d < 0 ? 0 : (d > 2 * p.R ? 2 * p.R : d)];
        }
    }

    // ---- Q^T fragments: lane (query li, kq) holds dims 8 kq .. + 7 (k-step 0) and 32 + 8 kq .. (k-step 1)
    const int qi = q0 + wave * 16 + li;
    f16x8 qh[2], ql[2];
    float iq, gq = 0.f;
    {
        f32x4 xa[2], xb[2];
        unsigned am = 0;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            xa[u] = xb[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (qi < p.T) {
                const float* src = base + (long long)qi * rs + 8 * kq + 4 * u;
                xa[u] = *reinterpret_cast<const f32x4*>(src);
                xb[u] = *reinterpret_cast<const f32x4*>(src + HD / 2);
            }
            amax_acc4(am, xa[u]);
            amax_acc4(am, xb[u]);
        }
        if (qi < p.T) gq = p.gate[((long long)b * gridDim.y + h) * p.T + qi];
        am = group_max_u32<64>(am);
        const int eq = s16_exponent(am);
        iq = s16_pow2(-eq);
        wl_pack8(xa[0], xa[1], s16_pow2(eq), qh[0], ql[0]);
        wl_pack8(xb[0], xb[1], s16_pow2(eq), qh[1], ql[1]);
    }

    // ---- staging registers of one key tile: K as (dims 4 g .., 32 + 4 g ..) pairs of two rows per thread, V as a 4-key x 4-dim block
    f32x4 kx0[2], kx1[2], vv[4];
    const int kg = tid >> 4, dg = tid & 15;
    auto issue_loads = [&](int kb) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e2 = tid + 256 * i, row = e2 >> 3, g = e2 & 7;
            const int t = kb + row;
            kx0[i] = kx1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < klim) {
                const float* src = base + (long long)t * rs + p.A + 4 * g;
                kx0[i] = *reinterpret_cast<const f32x4*>(src);
                kx1[i] = *reinterpret_cast<const f32x4*>(src + HD / 2);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = kb + 4 * kg + r;
            vv[r] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < klim) vv[r] = *reinterpret_cast<const f32x4*>(base + (long long)t * rs + 2 * p.A + 4 * dg);
        }
    };

    float m_run = -INFINITY, l_run = 0.f;
    f32x4 o[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};

    issue_loads(0);
    __syncthreads();                                           // the amax words are zero, the table is complete
    int jt = 0;
    for (int kb = 0; kb < klim; kb += KT, ++jt) {
        unsigned amk = 0, amv = 0;
#pragma unroll
        for (int i = 0; i < 2; ++i) { amax_acc4(amk, kx0[i]); amax_acc4(amk, kx1[i]); }
#pragma unroll
        for (int r = 0; r < 4; ++r) amax_acc4(amv, vv[r]);
        amk = group_max_u32<64>(amk);
        amv = group_max_u32<64>(amv);
        unsigned* sl = slot + (jt % 3) * 2;
        if (lane == 0) { atomicMax(sl, amk); atomicMax(sl + 1, amv); }
        __syncthreads();                                       // A: maxima complete; every wave is done with the previous tile's planes
        if (tid < 2) slot[((jt + 1) % 3) * 2 + tid] = 0u;      // (next tile's words: last read before the previous tile's barrier B)
        const int ek = s16_exponent(sl[0]), ev = s16_exponent(sl[1]);
        const float sk = s16_pow2(ek), svs = s16_pow2(ev);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e2 = tid + 256 * i, row = e2 >> 3, g = e2 & 7;
            split16_store4s(kx0[i], sk, Kp, PLANE, row * KP + 4 * g);
            split16_store4s(kx1[i], sk, Kp, PLANE, row * KP + HD / 2 + 4 * g);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)                            // V^T: four consecutive keys of one dim per 8-byte store
            split16_store4s(f32x4{vv[0][u], vv[1][u], vv[2][u], vv[3][u]}, svs, Vp, PLANE, (4 * dg + u) * KP + 4 * kg);
        if (kb + KT < klim) issue_loads(kb + KT);              // in flight during this tile's products
        __syncthreads();                                       // B: planes visible

        // ---- S^T = K Q^T: accumulator c, register r <-> key kb + 16 c + 4 kq + r, this lane's query
        f32x4 s[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const f16x8 kh = *reinterpret_cast<const f16x8*>(Kp + (c * 16 + li) * KP + 32 * ks + 8 * kq);
                const f16x8 kl = *reinterpret_cast<const f16x8*>(Kp + PLANE + (c * 16 + li) * KP + 32 * ks + 8 * kq);
                s[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], s[c], 0, 0, 0);
                s[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], s[c], 0, 0, 0);
                s[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], s[c], 0, 0, 0);
            }
        }
        // ---- bias, key limit, online softmax (lane-local but for the four kq groups of the query)
        const float ds = iq * s16_pow2(-ek) * p.scaling;
        const int tb = q0 + 63 - qi;                           // table index of delta = 0 for this query
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = kb + c * 16 + kq * 4 + r;
                float v = -INFINITY;
                if (j < klim) v = fmaf(gq, tab[tb + j], s[c][r] * ds);
                s[c][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);                  // finite: every tile of the loop holds a visible key
        const float alpha = __expf(m_run - m_new);             // exp(-inf) = 0 on the first tile
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = __expf(s[c][r] - m_new);
                s[c][r] = pv;
                sum += pv;
            }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        l_run = l_run * alpha + sum;
        m_run = m_new;
        // ---- O^T += V^T P^T, the tile's contribution in its own units first
        f32x4 tacc[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) tacc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 ph, pl;
            wl_pack8(s[2 * kk], s[2 * kk + 1], 16384.0f, ph, pl);
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const _Float16* vr = Vp + (d * 16 + li) * KP + 32 * kk + 4 * kq;
                const f16x4_t vh0 = *reinterpret_cast<const f16x4_t*>(vr), vh1 = *reinterpret_cast<const f16x4_t*>(vr + 16);
                const f16x4_t vl0 = *reinterpret_cast<const f16x4_t*>(vr + PLANE), vl1 = *reinterpret_cast<const f16x4_t*>(vr + PLANE + 16);
                const f16x8 vh = __builtin_shufflevector(vh0, vh1, 0, 1, 2, 3, 4, 5, 6, 7);
                const f16x8 vl = __builtin_shufflevector(vl0, vl1, 0, 1, 2, 3, 4, 5, 6, 7);
                tacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, tacc[d], 0, 0, 0);
                tacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, tacc[d], 0, 0, 0);
                tacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, tacc[d], 0, 0, 0);
            }
        }
        const float dv = s16_pow2(-ev) * (1.0f / 16384.0f);
#pragma unroll
        for (int d = 0; d < 4; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[d][r] = __fmaf_rn(tacc[d][r], dv, o[d][r] * alpha);
    }
    // ---- normalise and store: this lane's query, dims 16 d + 4 kq .. + 3
    if (qi < p.T) {
        float* dst = p.out + ((long long)b * p.T + qi) * p.A + (long long)h * HD + 4 * kq;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            *reinterpret_cast<f32x4*>(dst + d * 16) = f32x4{o[d][0] / l_run, o[d][1] / l_run, o[d][2] / l_run, o[d][3] / l_run};
    }
}

// ---------------------------------------------------------------------------------------------
// small element-wise and reduction kernels
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void spk_axpy_kernel(const f32x4* __restrict__ x, f32x4* __restrict__ acc, float w, int first, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 v = x[i];
        f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!first) a = acc[i];
        a.x = first ? __fmul_rn(w, v.x) : __fadd_rn(a.x, __fmul_rn(w, v.x));      // hidden * weight, then the sum over layers, unfused as the backend
        a.y = first ? __fmul_rn(w, v.y) : __fadd_rn(a.y, __fmul_rn(w, v.y));
        a.z = first ? __fmul_rn(w, v.z) : __fadd_rn(a.z, __fmul_rn(w, v.z));
        a.w = first ? __fmul_rn(w, v.w) : __fadd_rn(a.w, __fmul_rn(w, v.w));
        acc[i] = a;
    }
}

__global__ __launch_bounds__(256) void spk_relu_kernel(f32x4* __restrict__ x, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        f32x4 v = x[i];
        v.x = v.x > 0.f ? v.x : (v.x != v.x ? v.x : 0.f);      // (NaN stays NaN, as torch.relu)
        v.y = v.y > 0.f ? v.y : (v.y != v.y ? v.y : 0.f);
        v.z = v.z > 0.f ? v.z : (v.z != v.z ? v.z : 0.f);
        v.w = v.w > 0.f ? v.w : (v.w != v.w ? v.w : 0.f);
        x[i] = v;
    }
}

// x [B][M][C] -> out [B][2 C]: mean | unbiased std over the rows [0, lens[2 b + 1]) of clip b, two passes, one thread per (clip, channel).
// One row gives 0 / 0 = NaN (torch.std of one element); none gives NaN too.
__global__ __launch_bounds__(256) void spk_pool_kernel(const float* __restrict__ x, const int* __restrict__ lens, int M, int C, float* __restrict__ out) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int n = min(lens[2 * b + 1], M);
    const float* xb = x + (long long)b * M * C + c;
    float mean = NAN, sd = NAN;
    if (n >= 1) {
        float sum = 0.f;
        for (int t = 0; t < n; ++t) sum += xb[(long long)t * C];
        mean = sum / (float)n;
        float m2 = 0.f;
        for (int t = 0; t < n; ++t) {
            const float d = xb[(long long)t * C] - mean;
            m2 = fmaf(d, d, m2);
        }
        sd = sqrtf(m2 / (float)(n - 1));
    }
    out[(long long)b * 2 * C + c] = mean;
    out[(long long)b * 2 * C + C + c] = sd;
}

// one wave per pair
__global__ __launch_bounds__(256) void spk_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int D, float* __restrict__ out) {
    const int pair = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (pair >= B) return;
    const float* ar = a + (long long)pair * D;
    const float* br = b + (long long)pair * D;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int i = lane; i < D; i += 64) {
        const float u = ar[i], v = br[i];
        ab = fmaf(u, v, ab);
        aa = fmaf(u, u, aa);
        bb = fmaf(v, v, bb);
    }
#pragma unroll
    for (int sh = 1; sh < 64; sh <<= 1) {
        ab += __shfl_xor(ab, sh);
        aa += __shfl_xor(aa, sh);
        bb += __shfl_xor(bb, sh);
    }
    if (lane == 0) out[pair] = ab / (fmaxf(sqrtf(aa), 1e-8f) * fmaxf(sqrtf(bb), 1e-8f));
}

}  // namespace ac
