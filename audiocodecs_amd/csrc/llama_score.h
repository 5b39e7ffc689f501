// llama_score.h: the kernels of the full-sequence (teacher-forced) Llama forward that scores token sequences (lm_score.hip, DESIGN.md
// section 8r).  The linear layers are linear_rows (core.hip: the split16 tap-GEMM in row mode); what this header adds is everything
// between them.  Plain launches only: no kernel waits for another workgroup or counts arrivals, and no float atomic exists, so a repeat
// is bit-identical.  Every scale is a row's, a query tile's or a key tile's of ONE clip: a clip's result does not depend on its batch.
//
//   lm_norm_rows_kernel      y = x rsqrt(mean(x^2) + eps) w per row, and the row's amax word for linear_rows (Epi::rowmax_in)
//   lm_rope_rows_kernel      the interleaved pairs (2i, 2i + 1) of the q and k columns of the stacked [rows][q | k | v] matrix rotated in
//                            place by row `pos` (the row's index inside its clip) of the uploaded table
//   lm_swiglu_rows_kernel    silu(a) b from the stacked [rows][w1 x | w3 x], and the row's amax word
//   lm_attn16_causal_kernel  wavlm_attn16_kernel's scheme (wavlm.h; mimi.h has the derivation): S^T = K Q^T and O^T = V^T P^T on
//                            v_mfma_f32_16x16x32_f16 in split16 arithmetic, one query per lane, online softmax, no score in memory --
//                            causal, head dim HD (a multiple of 16 up to 128; 16 is padded to the 32 of a k-step with zeros), and
//                            grouped: a workgroup is the G query heads of ONE key/value head on the same 16 queries, one head per wave,
//                            and all of them read the K and V^T planes of a 64-key tile that the workgroup staged once.  Key tiles wholly
//                            above the diagonal are never visited; the others are masked per element.  Grid (ceil(T / 16), kv heads, clips).
//   lm_score_head_kernel     the rows of one codebook against that codebook's output head, the vocabulary walked in tiles of 16 columns
//                            on the same MFMA (logits^T = W X^T: a lane owns one row).  Per row only the running maximum, the sum of
//                            exponentials, the target's logit and the arg-max survive: log-prob and prediction are written, logits only
//                            when the caller asks for the stage.
//   lm_score_reduce_kernel   sum of log-probs (fp64, fixed order), scored positions and errors per clip: one workgroup per clip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "split16.h"

namespace ac {

typedef float ls_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float ls_wave_sum(float x) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) x += __shfl_xor(x, sh);
    return x;
}

// 8 fp32 (two quads) x scale -> the hi / lo fp16 fragments of one MFMA operand (split16.h: scaled value = hi + lo)
__device__ __forceinline__ void ls_pack8(const ls_f32x4 a, const ls_f32x4 b, const float sc, f16x8& hi, f16x8& lo) {
    const ls_f32x4 s0 = a * sc, s1 = b * sc;
    const f16x4_t h0 = __builtin_convertvector(s0, f16x4_t), h1 = __builtin_convertvector(s1, f16x4_t);
    const f16x4_t l0 = __builtin_convertvector(s0 - __builtin_convertvector(h0, ls_f32x4), f16x4_t);
    const f16x4_t l1 = __builtin_convertvector(s1 - __builtin_convertvector(h1, ls_f32x4), f16x4_t);
    hi = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
    lo = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// n4 float4s
__global__ __launch_bounds__(256) void lm_copy4_kernel(const ls_f32x4* __restrict__ src, ls_f32x4* __restrict__ dst, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

// ---- RMSNorm of a row (one wave per row, dim % 4 == 0) ---------------------------------------------------------------------------------
struct LmNormRows {
    const float* x;      // [rows][dim]
    const float* w;      // [dim]
    float* y;            // [rows][dim]
    unsigned* rowmax;    // [rows] or null: bits of the largest finite |y| of the row (split16.h row mode)
    long long rows;
    int dim;
    float eps;
};

__global__ __launch_bounds__(256) void lm_norm_rows_kernel(const LmNormRows p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float* xr = p.x + row * p.dim;
    float ss = 0.0f;
    for (int d = lane * 4; d < p.dim; d += 256) {
        const ls_f32x4 v = *reinterpret_cast<const ls_f32x4*>(xr + d);
        ss = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, ss))));
    }
    const float rs = rsqrtf(ls_wave_sum(ss) / (float)p.dim + p.eps);
    float* yr = p.y + row * p.dim;
    unsigned mx = 0;
    for (int d = lane * 4; d < p.dim; d += 256) {
        const ls_f32x4 v = *reinterpret_cast<const ls_f32x4*>(xr + d), g = *reinterpret_cast<const ls_f32x4*>(p.w + d);
        const ls_f32x4 o = ls_f32x4{v.x * rs * g.x, v.y * rs * g.y, v.z * rs * g.z, v.w * rs * g.w};
        *reinterpret_cast<ls_f32x4*>(yr + d) = o;
        amax_acc4(mx, o);
    }
    if (p.rowmax) {
        mx = group_max_u32<64>(mx);
        if (lane == 0) p.rowmax[row] = mx;
    }
}

// ---- RoPE in place on the q and k columns of [rows][pitch]: one workgroup per row, a thread per pair ----------------------------------
struct LmRopeRows {
    float* qkv;          // [clips * T][pitch]: q (nq) | k (nkvd) | v
    const float* rcos;   // [table rows][hd / 2]
    const float* rsin;
    int T, pitch, nqk, hd;   // nqk = nq + nkvd: the rotated columns
};

__global__ __launch_bounds__(256) void lm_rope_rows_kernel(const LmRopeRows p) {
    const long long row = blockIdx.x;
    const int pos = (int)(row % p.T), half = p.hd / 2;
    float* r = p.qkv + row * p.pitch;
    for (int j = threadIdx.x; j < p.nqk / 2; j += 256) {
        const int f = j % half;
        const float cs = p.rcos[(size_t)pos * half + f], sn = p.rsin[(size_t)pos * half + f];
        const float a = r[2 * j], b = r[2 * j + 1];
        r[2 * j] = a * cs - b * sn;
        r[2 * j + 1] = a * sn + b * cs;
    }
}

// ---- silu(a) * b (one wave per row, F % 4 == 0) ----------------------------------------------------------------------------------------
struct LmSwigluRows {
    const float* h2;     // [rows][2 F]: w1 x | w3 x
    float* y;            // [rows][F]
    unsigned* rowmax;    // [rows] or null
    long long rows;
    int F;
};

__global__ __launch_bounds__(256) void lm_swiglu_rows_kernel(const LmSwigluRows p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float* a = p.h2 + row * 2 * p.F;
    const float* b = a + p.F;
    float* yr = p.y + row * p.F;
    unsigned mx = 0;
    for (int d = lane * 4; d < p.F; d += 256) {
        const ls_f32x4 u = *reinterpret_cast<const ls_f32x4*>(a + d), v = *reinterpret_cast<const ls_f32x4*>(b + d);
        const ls_f32x4 o = ls_f32x4{u.x / (1.0f + expf(-u.x)) * v.x, u.y / (1.0f + expf(-u.y)) * v.y, u.z / (1.0f + expf(-u.z)) * v.z,
                                    u.w / (1.0f + expf(-u.w)) * v.w};
        *reinterpret_cast<ls_f32x4*>(yr + d) = o;
        amax_acc4(mx, o);
    }
    if (p.rowmax) {
        mx = group_max_u32<64>(mx);
        if (lane == 0) p.rowmax[row] = mx;
    }
}

// ---- causal grouped-query attention ----------------------------------------------------------------------------------------------------
struct LmAttn16 {
    const float* qkv;    // [clips][T][pitch]: q (nq, rotated) | k (nkvd, rotated) | v (nkvd)
    float* out;          // [clips][T][nq]
    int T, pitch, nq, nkvd, G;     // G query heads per key/value head = waves of a workgroup
    float scale;
};

template <int HD>
struct LmAttn16Cfg {
    static_assert(HD % 16 == 0 && HD >= 16 && HD <= 128, "head dim: a multiple of 16 up to 128");
    static constexpr int QT = 16, KT = 64;
    static constexpr int HDP = (HD + 31) / 32 * 32;      // dims of the first product's k-steps (32 each)
    static constexpr int KS = HDP / 32, ND = HD / 16;
    static constexpr int KP = HDP + 8, VP = KT + 8;      // fp16 per LDS row: K [key][dim], V^T [dim][key]
    static constexpr int KPLANE = KT * KP, VPLANE = HD * VP;
    static constexpr size_t lds_bytes = (size_t)(2 * KPLANE + 2 * VPLANE) * 2 + 32;
};

template <int HD>
__global__ __launch_bounds__(512) void lm_attn16_causal_kernel(const LmAttn16 p) {
    using Cfg = LmAttn16Cfg<HD>;
    constexpr int KT = Cfg::KT, HDP = Cfg::HDP, KS = Cfg::KS, ND = Cfg::ND, KP = Cfg::KP, VP = Cfg::VP, KPLANE = Cfg::KPLANE, VPLANE = Cfg::VPLANE;
    constexpr int C4 = HD / 4;                                       // float4s of a key row
    extern __shared__ __attribute__((aligned(16))) float smem[];
    _Float16* Kp = reinterpret_cast<_Float16*>(smem);                // [2 planes][64 keys][KP]
    _Float16* Vp = Kp + 2 * KPLANE;                                  // [2 planes][HD dims][VP]  (keys along the row)
    unsigned* slot = reinterpret_cast<unsigned*>(Vp + 2 * VPLANE);   // [3 rotating][K, V]

    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * Cfg::QT, g = blockIdx.y, b = blockIdx.z;
    const int head = g * p.G + wave;
    const float* base = p.qkv + (long long)b * p.T * p.pitch;
    const float* kbase = base + p.nq + g * HD;
    const float* vbase = kbase + p.nkvd;
    if (tid < 6) slot[tid] = 0u;
    if constexpr (HDP > HD) {                                        // the k-step's dims beyond the head: zero in both planes, never rewritten
        for (int i = tid; i < 2 * KT * (HDP - HD); i += nt) {
            const int pl = i / (KT * (HDP - HD)), r = i % (KT * (HDP - HD));
            Kp[pl * KPLANE + (r / (HDP - HD)) * KP + HD + r % (HDP - HD)] = (_Float16)0.0f;
        }
    }

    // ---- Q^T fragments: lane (query li, kq) holds dims 32 ks + 8 kq .. + 7 of k-step ks; one scale per wave (16 queries of one head)
    const int qi = q0 + li;
    f16x8 qh[KS], ql[KS];
    float iq;
    {
        ls_f32x4 xa[KS][2];
        unsigned am = 0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int d = 32 * ks + 8 * kq + 4 * u;
                xa[ks][u] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
                if (qi < p.T && d < HD) xa[ks][u] = *reinterpret_cast<const ls_f32x4*>(base + (long long)qi * p.pitch + head * HD + d);
                amax_acc4(am, xa[ks][u]);
            }
        am = group_max_u32<64>(am);
        const int eq = s16_exponent(am);
        iq = s16_pow2(-eq);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) ls_pack8(xa[ks][0], xa[ks][1], s16_pow2(eq), qh[ks], ql[ks]);
    }

    float m_run = -INFINITY, l_run = 0.f;
    ls_f32x4 o[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d) o[d] = ls_f32x4{0.f, 0.f, 0.f, 0.f};

    const int q_last = min(q0 + Cfg::QT - 1, p.T - 1);
    __syncthreads();                                                 // the amax words and the padding are zero
    int jt = 0;
    // (kb <= q0 for every tile of the loop: both are multiples of 16, so each query of the workgroup sees at least key kb of it)
    for (int kb = 0; kb <= q_last; kb += KT, ++jt) {
        // ---- pass 1: the tile's largest |k| and |v| (rows at and beyond T count as zero)
        unsigned amk = 0, amv = 0;
        for (int i = tid; i < KT * C4; i += nt) {
            const int t = kb + i / C4, c4 = i % C4;
            if (t < p.T) {
                amax_acc4(amk, *reinterpret_cast<const ls_f32x4*>(kbase + (long long)t * p.pitch + 4 * c4));
                amax_acc4(amv, *reinterpret_cast<const ls_f32x4*>(vbase + (long long)t * p.pitch + 4 * c4));
            }
        }
        amk = group_max_u32<64>(amk);
        amv = group_max_u32<64>(amv);
        unsigned* sl = slot + (jt % 3) * 2;
        if (lane == 0) { atomicMax(sl, amk); atomicMax(sl + 1, amv); }
        __syncthreads();                                             // A: maxima complete; every wave is done with the previous tile's planes
        if (tid < 2) slot[((jt + 1) % 3) * 2 + tid] = 0u;            // (next tile's words: last read before the previous tile's barrier B)
        const int ek = s16_exponent(sl[0]), ev = s16_exponent(sl[1]);
        const float sk = s16_pow2(ek), svs = s16_pow2(ev);
        // ---- pass 2: the planes (the rows come from the cache this time)
        for (int i = tid; i < KT * C4; i += nt) {
            const int row = i / C4, c4 = i % C4, t = kb + row;
            ls_f32x4 kx = ls_f32x4{0.f, 0.f, 0.f, 0.f};
            if (t < p.T) kx = *reinterpret_cast<const ls_f32x4*>(kbase + (long long)t * p.pitch + 4 * c4);
            split16_store4s(kx, sk, Kp, KPLANE, row * KP + 4 * c4);
        }
        for (int i = tid; i < (KT / 4) * C4; i += nt) {              // V^T: a 4-key x 4-dim block per thread, four keys of one dim per 8-byte store
            const int kg = i / C4, dg = i % C4;
            ls_f32x4 vv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = kb + 4 * kg + r;
                vv[r] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
                if (t < p.T) vv[r] = *reinterpret_cast<const ls_f32x4*>(vbase + (long long)t * p.pitch + 4 * dg);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) split16_store4s(ls_f32x4{vv[0][u], vv[1][u], vv[2][u], vv[3][u]}, svs, Vp, VPLANE, (4 * dg + u) * VP + 4 * kg);
        }
        __syncthreads();                                             // B: planes visible

        // ---- S^T = K Q^T: accumulator c, register r <-> key kb + 16 c + 4 kq + r, this lane's query
        ls_f32x4 s[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s[c] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const f16x8 kh = *reinterpret_cast<const f16x8*>(Kp + (c * 16 + li) * KP + 32 * ks + 8 * kq);
                const f16x8 kl = *reinterpret_cast<const f16x8*>(Kp + KPLANE + (c * 16 + li) * KP + 32 * ks + 8 * kq);
                s[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[ks], s[c], 0, 0, 0);
                s[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[ks], s[c], 0, 0, 0);
                s[c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[ks], s[c], 0, 0, 0);
            }
        }
        // ---- the diagonal, online softmax (lane-local but for the four kq groups of the query)
        const float ds = iq * s16_pow2(-ek) * p.scale;
        float mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = kb + c * 16 + kq * 4 + r;
                const float v = j <= qi ? s[c][r] * ds : -INFINITY;
                s[c][r] = v;
                mx = fmaxf(mx, v);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);                        // finite: key kb is visible to every query
        const float alpha = __expf(m_run - m_new);                   // exp(-inf) = 0 on the first tile
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
        ls_f32x4 tacc[ND];
#pragma unroll
        for (int d = 0; d < ND; ++d) tacc[d] = ls_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            f16x8 ph, pl;
            ls_pack8(s[2 * kk], s[2 * kk + 1], 16384.0f, ph, pl);
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                const _Float16* vr = Vp + (d * 16 + li) * VP + 32 * kk + 4 * kq;
                const f16x4_t vh0 = *reinterpret_cast<const f16x4_t*>(vr), vh1 = *reinterpret_cast<const f16x4_t*>(vr + 16);
                const f16x4_t vl0 = *reinterpret_cast<const f16x4_t*>(vr + VPLANE), vl1 = *reinterpret_cast<const f16x4_t*>(vr + VPLANE + 16);
                const f16x8 vh = __builtin_shufflevector(vh0, vh1, 0, 1, 2, 3, 4, 5, 6, 7);
                const f16x8 vl = __builtin_shufflevector(vl0, vl1, 0, 1, 2, 3, 4, 5, 6, 7);
                tacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, tacc[d], 0, 0, 0);
                tacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, tacc[d], 0, 0, 0);
                tacc[d] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, tacc[d], 0, 0, 0);
            }
        }
        const float dv = s16_pow2(-ev) * (1.0f / 16384.0f);
#pragma unroll
        for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[d][r] = __fmaf_rn(tacc[d][r], dv, o[d][r] * alpha);
    }
    // ---- normalise and store: this lane's query, dims 16 d + 4 kq .. + 3
    if (qi < p.T) {
        float* dst = p.out + ((long long)b * p.T + qi) * p.nq + head * HD + 4 * kq;
#pragma unroll
        for (int d = 0; d < ND; ++d)
            *reinterpret_cast<ls_f32x4*>(dst + d * 16) = ls_f32x4{o[d][0] / l_run, o[d][1] / l_run, o[d][2] / l_run, o[d][3] / l_run};
    }
}

// ---- the output head that keeps no logits ----------------------------------------------------------------------------------------------
struct LmScoreHead {
    const float* xn;             // [clips][Ttot][dim]: the final norm
    const _Float16* img;         // this codebook's head: [Cpad / 16][KS][plane 2][lane 64][8] (Packer::frag16)
    const float* winv;           // [Cpad]: 2^-s of its rows
    const long long* targets;    // [clips][T]
    const long long* lengths;    // [clips] or null
    float* logp;                 // [clips][T]
    long long* pred;             // [clips][T]
    float* logits;               // [clips][T][C] or null
    int clips, T, P, dim, C, ncb, k, KS, ntiles, Tk;   // Tk = rows of codebook k per clip: t = k + j ncb
};

constexpr int LSH_ROWS = 16;
constexpr int LSH_COMB = 8;      // words per (wave, row) of the merge area
inline size_t lm_score_head_lds(int KS) { return (size_t)2 * LSH_ROWS * (KS * 32 + 8) * 2 + (size_t)4 * LSH_ROWS * LSH_COMB * 4 + LSH_ROWS * 4; }

// (m, s) of a softmax denominator and the arg-max (v, i), merged with another part's; the lower index wins a tie
__device__ __forceinline__ void ls_merge(float& m, float& s, float& tl, float& bv, int& bi, float m2, float s2, float tl2, float bv2, int bi2) {
    const float M = fmaxf(m, m2);
    const float f1 = m == M ? 1.0f : expf(m - M), f2 = m2 == M ? 1.0f : expf(m2 - M);      // (equal covers -inf against -inf)
    s = s * f1 + s2 * f2;
    m = M;
    tl = fmaxf(tl, tl2);
    if (bv2 > bv || (bv2 == bv && bi2 < bi)) { bv = bv2; bi = bi2; }
}

// 16 rows per workgroup; the four waves share the rows' split16 planes in LDS and take every fourth vocabulary tile each
__global__ __launch_bounds__(256) void lm_score_head_kernel(const LmScoreHead p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int XP = p.KS * 32 + 8, XPLANE = LSH_ROWS * XP;
    _Float16* Xp = reinterpret_cast<_Float16*>(smem);                          // [2 planes][16 rows][XP]
    float* comb = reinterpret_cast<float*>(Xp + 2 * XPLANE);                   // [4 waves][16 rows][LSH_COMB]
    float* ixs = comb + 4 * LSH_ROWS * LSH_COMB;                               // [16]: 2^-s of the rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, kq = lane >> 4;
    const long long Mk = (long long)p.clips * p.Tk, m0 = (long long)blockIdx.x * LSH_ROWS;
    const int Ttot = p.P + p.T;
    // ---- the rows 4 wave .. + 3 into the planes, each under its own scale
    for (int r = 4 * wave; r < 4 * wave + 4; ++r) {
        const long long m = m0 + r;
        const bool valid = m < Mk;
        const long long bb = valid ? m / p.Tk : 0;
        const int t = valid ? p.k + (int)(m - bb * p.Tk) * p.ncb : 0;
        const float* xr = p.xn + (bb * Ttot + p.P + t) * p.dim;
        unsigned am = 0;
        if (valid)
            for (int d = lane * 4; d < p.dim; d += 256) amax_acc4(am, *reinterpret_cast<const ls_f32x4*>(xr + d));
        am = group_max_u32<64>(am);
        const int e = s16_exponent(am);
        const float sc = s16_pow2(e);
        for (int d = lane * 4; d < p.KS * 32; d += 256) {
            ls_f32x4 v = ls_f32x4{0.f, 0.f, 0.f, 0.f};
            if (valid && d < p.dim) v = *reinterpret_cast<const ls_f32x4*>(xr + d);
            split16_store4s(v, sc, Xp, XPLANE, r * XP + d);
        }
        if (lane == 0) ixs[r] = s16_pow2(-e);
    }
    __syncthreads();
    // ---- this lane's row: li
    const long long m = m0 + li;
    const bool valid = m < Mk;
    const long long bb = valid ? m / p.Tk : 0;
    const int t = valid ? p.k + (int)(m - bb * p.Tk) * p.ncb : 0;
    const long long at = bb * p.T + t;
    const long long tgt = valid ? p.targets[at] : -1;
    const float ix = ixs[li];
    float mr = -INFINITY, sr = 0.0f, tl = -INFINITY, bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int nt = wave; nt < p.ntiles; nt += 4) {
        ls_f32x4 acc = ls_f32x4{0.f, 0.f, 0.f, 0.f};
        const _Float16* wt = p.img + ((size_t)nt * p.KS * 2) * 512 + (size_t)lane * 8;
        for (int ks = 0; ks < p.KS; ++ks) {
            const f16x8 wh = *reinterpret_cast<const f16x8*>(wt + (size_t)ks * 1024);
            const f16x8 wl = *reinterpret_cast<const f16x8*>(wt + (size_t)ks * 1024 + 512);
            const f16x8 xh = *reinterpret_cast<const f16x8*>(Xp + li * XP + 32 * ks + 8 * kq);
            const f16x8 xl = *reinterpret_cast<const f16x8*>(Xp + XPLANE + li * XP + 32 * ks + 8 * kq);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, xh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, xh, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nt * 16 + kq * 4 + r;
            if (n >= p.C) continue;
            const float v = acc[r] * (ix * p.winv[n]);
            if (p.logits && valid) p.logits[at * p.C + n] = v;
            if (v > mr) {
                sr = sr * expf(mr - v) + 1.0f;                                 // (exp(-inf) = 0 at the first column)
                mr = v;
            } else {
                sr += expf(v - mr);
            }
            if (n == tgt) tl = v;
            if (v > bv) { bv = v; bi = n; }                                    // (columns come in rising order: the first maximum stays)
        }
    }
    // ---- the four kq groups of the row, then the four waves, in a fixed order
#pragma unroll
    for (int sh = 16; sh <= 32; sh <<= 1)
        ls_merge(mr, sr, tl, bv, bi, __shfl_xor(mr, sh), __shfl_xor(sr, sh), __shfl_xor(tl, sh), __shfl_xor(bv, sh), __shfl_xor(bi, sh));
    if (kq == 0) {
        float* c = comb + (wave * LSH_ROWS + li) * LSH_COMB;
        c[0] = mr; c[1] = sr; c[2] = tl; c[3] = bv;
        reinterpret_cast<int*>(c)[4] = bi;
    }
    __syncthreads();
    if (tid < LSH_ROWS && valid) {
        const float* c = comb + tid * LSH_COMB;
        float M = c[0], S = c[1], TL = c[2], BV = c[3];
        int BI = reinterpret_cast<const int*>(c)[4];
        for (int w = 1; w < 4; ++w) {
            const float* cw = comb + (w * LSH_ROWS + tid) * LSH_COMB;
            ls_merge(M, S, TL, BV, BI, cw[0], cw[1], cw[2], cw[3], reinterpret_cast<const int*>(cw)[4]);
        }
        long long len = p.T;
        if (p.lengths) { len = p.lengths[bb]; len = len < 0 ? 0 : len > p.T ? p.T : len; }
        const bool scored = tgt >= 0 && tgt < p.C && t < len;
        p.logp[at] = scored ? TL - M - logf(S) : 0.0f;
        p.pred[at] = BI;
    }
}

// ---- sums per clip: one workgroup per clip, a contiguous run of positions per thread, the 256 partial sums added in order ---------------
struct LmScoreReduce {
    const float* logp;           // [B][T]
    const long long* pred;
    const long long* targets;
    const long long* lengths;    // [B] or null
    double* sum_logp;            // [B]
    long long* count;
    long long* errors;
    int T, C;
};

__global__ __launch_bounds__(256) void lm_score_reduce_kernel(const LmScoreReduce p) {
    __shared__ double ssum[256];
    __shared__ long long scnt[256], serr[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    long long len = p.T;
    if (p.lengths) { len = p.lengths[b]; len = len < 0 ? 0 : len > p.T ? p.T : len; }
    const int per = (p.T + 255) / 256, t0 = tid * per, t1 = min(t0 + per, p.T);
    double s = 0.0;
    long long n = 0, e = 0;
    for (int t = t0; t < t1; ++t) {
        const long long at = (long long)b * p.T + t, tg = p.targets[at];
        if (tg >= 0 && tg < p.C && t < len) {
            s += (double)p.logp[at];
            n += 1;
            e += p.pred[at] != tg ? 1 : 0;
        }
    }
    ssum[tid] = s; scnt[tid] = n; serr[tid] = e;
    __syncthreads();
    if (tid == 0) {
        double S = 0.0;
        long long N = 0, E = 0;
        for (int i = 0; i < 256; ++i) { S += ssum[i]; N += scnt[i]; E += serr[i]; }
        p.sum_logp[b] = S; p.count[b] = N; p.errors[b] = E;
    }
}

}  // namespace ac
