// The TokenProbe's kernels beside the recurrence (bilstm.h) and the matrix products (linear_rows): DESIGN.md section 8s.  Plain launches
// in one linear chain; no kernel waits for another workgroup, nothing is counted between workgroups and no float atomic exists, so a
// repeat is bit-identical.  Every row, scale and scan belongs to ONE clip: a clip's result does not depend on its batch or its chunk.
//
//   probe_zero_kernel        float4 zero fill: the layers' outputs and the recurrent state of a chunk, once per call and chunk
//   probe_embed_pool_kernel  toks [rows][K] -> pooled [rows][E] and the row's amax word for linear_rows (Epi::rowmax_in): the K table rows
//                            of a frame are gathered and summed under the pooling's weights in one pass, one wave per frame; the
//                            [B][N][K][E] tensor of the reference never exists.  LinearPooling: the weights are the layer's K numbers.
//                            AttentionalPooling: the score of a code depends on its id alone, so it is a table folded at load; the kernel
//                            gathers K scores and takes their softmax.
//   probe_ctc_rows_kernel    a row of logits -> max, sum of exponentials, arg-max (lowest index on a tie); frame_pred, optional log_probs
//   probe_ctc_collapse_kernel one workgroup per clip: keep[t] = pred[t] != pred[t-1] && pred[t] != blank && t < L, compacted by scan
//   probe_utt_head_kernel    one workgroup per clip: mean and unbiased std over the valid frames (fp64, frame order), the dense layer and
//                            log_softmax in fp32, the arg-max
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bilstm.h"
#include "split16.h"

namespace ac {

constexpr int PROBE_MAX_K = 32;      // codebooks per frame: one lane each in the pooling kernel

__global__ __launch_bounds__(256) void probe_zero_kernel(s16_f32x4* __restrict__ p, long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) p[i] = s16_f32x4{0.f, 0.f, 0.f, 0.f};
}

struct ProbeEmbedPool {
    const long long* toks;   // [rows][K]
    const float* table;      // [K C (+ 1)][E]
    const float* wlin;       // [K] LinearPooling weights, or null
    const float* score;      // [K C + 2] AttentionalPooling scores (entry K C: the padding row, K C + 1: a zero row), or null
    float* out;              // [rows][E]
    unsigned* rowmax;        // [rows]
    unsigned* bad;           // the handle's ST_BAD_TOKEN word
    long long rows;
    int K, C, E, padding;
};

__global__ __launch_bounds__(256) void probe_embed_pool_kernel(const ProbeEmbedPool p) {
    __shared__ long long sidx[4][PROBE_MAX_K];      // table row of codebook k, -1: an id out of range (a zero row)
    __shared__ float sw[4][PROBE_MAX_K];            // its score, then its weight
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    const bool live = row < p.rows;
    bool bad = false;
    if (live && lane < p.K) {                        // lane k reads codebook k's id
        const long long id = p.toks[row * p.K + lane];
        long long r = -1;
        if (id >= 0 && id < p.C) r = (long long)lane * p.C + id;
        else if (p.padding && id == p.C) r = (long long)p.K * p.C;
        else bad = true;
        sidx[wave][lane] = r;
        sw[wave][lane] = p.score ? p.score[r >= 0 ? r : (long long)p.K * p.C + 1] : (p.wlin ? p.wlin[lane] : 1.0f);
    }
    const int nbad = __popcll(__ballot(bad));
    if (nbad && lane == 0 && p.bad) atomicAdd(p.bad, (unsigned)nbad);
    __syncthreads();
    float wk = 0.f;
    if (live && p.score && lane < p.K) {             // the softmax over the K scores, summed in codebook order
        float m = -INFINITY, sum = 0.f;
        for (int k = 0; k < p.K; ++k) m = fmaxf(m, sw[wave][k]);
        for (int k = 0; k < p.K; ++k) sum += expf(sw[wave][k] - m);
        wk = expf(sw[wave][lane] - m) / sum;
    }
    __syncthreads();
    if (live && p.score && lane < p.K) sw[wave][lane] = wk;
    __syncthreads();
    if (!live) return;
    float* o = p.out + row * p.E;
    unsigned mx = 0;
    for (int d = lane * 4; d < p.E; d += 256) {
        s16_f32x4 acc = s16_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < p.K; ++k) {
            const long long r = sidx[wave][k];
            if (r < 0) continue;
            const float w = sw[wave][k];
            const s16_f32x4 v = *reinterpret_cast<const s16_f32x4*>(p.table + r * p.E + d);
            acc.x = fmaf(v.x, w, acc.x); acc.y = fmaf(v.y, w, acc.y); acc.z = fmaf(v.z, w, acc.z); acc.w = fmaf(v.w, w, acc.w);
        }
        *reinterpret_cast<s16_f32x4*>(o + d) = acc;
        amax_acc4(mx, acc);
    }
    mx = group_max_u32<64>(mx);
    if (lane == 0) p.rowmax[row] = mx;
}

// (m, s) of a softmax denominator and the arg-max (v, i) merged across the wave; the lower index wins a tie
__device__ __forceinline__ void probe_wave_softmax_argmax(float& m, float& s, float& v, int& i) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const float m2 = __shfl_xor(m, sh), s2 = __shfl_xor(s, sh), v2 = __shfl_xor(v, sh);
        const int i2 = __shfl_xor(i, sh);
        const float mn = fmaxf(m, m2);
        // (a lane without an element has m = -inf and s = 0: its term is dropped rather than exponentiated to NaN)
        const float t1 = m == -INFINITY ? 0.f : s * expf(m - mn), t2 = m2 == -INFINITY ? 0.f : s2 * expf(m2 - mn);
        // the two terms are added in the order of their lanes, so that both partners hold the same bits
        s = (threadIdx.x & sh) ? t2 + t1 : t1 + t2;
        m = mn;
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
    }
}

struct ProbeCtcRows {
    const float* logits;       // [B][N][pitch]
    const long long* lengths;  // [B] or null
    long long* frame_pred;     // [B][N]
    float* log_probs;          // [B][N][C] or null
    int B, N, C, pitch;
};

__global__ __launch_bounds__(256) void probe_ctc_rows_kernel(const ProbeCtcRows p) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)p.B * p.N) return;
    const int b = (int)(row / p.N), t = (int)(row % p.N);
    const bool valid = t < probe_len(p.lengths, b, p.N);
    const float* x = p.logits + row * p.pitch;
    float m = -INFINITY, s = 0.f, v = -INFINITY;
    int i = 0x7fffffff;
    for (int c = lane; c < p.C; c += 64) {
        const float l = x[c];
        if (l > v || (l == v && c < i) || i == 0x7fffffff) { v = l; i = c; }
        const float mn = fmaxf(m, l);
        s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + expf(l - mn);
        m = mn;
    }
    probe_wave_softmax_argmax(m, s, v, i);
    if (lane == 0) p.frame_pred[row] = valid ? (long long)i : -1LL;
    if (p.log_probs) {
        const float lse = m + logf(s);
        float* o = p.log_probs + row * p.C;
        for (int c = lane; c < p.C; c += 64) o[c] = valid ? x[c] - lse : 0.f;
    }
}

struct ProbeCollapse {
    const long long* frame_pred;   // [B][N]: -1 beyond the clip's length
    long long* hyp_toks;           // [B][N]
    long long* hyp_lens;           // [B]
    int N;
    long long blank;
};

__global__ __launch_bounds__(256) void probe_ctc_collapse_kernel(const ProbeCollapse p) {
    __shared__ int scan[256];
    __shared__ int carry;
    const int tid = threadIdx.x;
    const long long* fp = p.frame_pred + (long long)blockIdx.x * p.N;
    long long* hyp = p.hyp_toks + (long long)blockIdx.x * p.N;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int t0 = 0; t0 < p.N; t0 += 256) {
        const int t = t0 + tid;
        long long cur = -1;
        int keep = 0;
        if (t < p.N) {
            cur = fp[t];
            const long long prev = t > 0 ? fp[t - 1] : -1;
            keep = cur >= 0 && cur != prev && cur != p.blank;      // (cur < 0: beyond the length)
        }
        scan[tid] = keep;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {                        // inclusive scan
            const int add = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        const int base = carry;
        if (keep) hyp[base + scan[tid] - 1] = cur;
        __syncthreads();
        if (tid == 255) carry = base + scan[255];
        __syncthreads();
    }
    const int count = carry;
    for (int t = count + tid; t < p.N; t += 256) hyp[t] = -1;
    if (tid == 0) p.hyp_lens[blockIdx.x] = count;
}

struct ProbeUttHead {
    const float* y;            // [B][N][F]: the last layer's output, F = 2H
    const long long* lengths;  // [B] or null
    const float* w;            // [C][2F]: mean columns, then std columns
    const float* bias;         // [C]
    float* logits_ws;          // [B][C] scratch
    float* logits_out;         // [B][C] or null (stage)
    float* log_probs;          // [B][C]
    long long* pred;           // [B]
    int N, F, C;
};

inline size_t probe_utt_lds(int F) { return (size_t)2 * F * sizeof(float); }

__global__ __launch_bounds__(256) void probe_utt_head_kernel(const ProbeUttHead p) {
    extern __shared__ float stats[];                // [2F]: mean | std
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const int L = probe_len(p.lengths, b, p.N);
    const float* yb = p.y + (long long)b * p.N * p.F;
    for (int f = tid; f < p.F; f += 256) {
        double sum = 0.0;
        for (int t = 0; t < L; ++t) sum += (double)yb[(long long)t * p.F + f];
        const double mean = sum / (double)L;        // L = 0: NaN, as torch
        double ss = 0.0;
        for (int t = 0; t < L; ++t) {
            const double d = (double)yb[(long long)t * p.F + f] - mean;
            ss += d * d;
        }
        stats[f] = (float)mean;
        stats[p.F + f] = (float)sqrt(ss / (double)(L - 1));   // L = 1: 0 / 0 = NaN, as torch's unbiased std
    }
    __syncthreads();
    float* lg = p.logits_ws + (long long)b * p.C;
    for (int c = wave; c < p.C; c += 4) {
        const float* wr = p.w + (long long)c * 2 * p.F;
        float acc = 0.f;
        for (int j = lane; j < 2 * p.F; j += 64) acc = fmaf(wr[j], stats[j], acc);
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) acc += __shfl_xor(acc, sh);
        if (lane == 0) {
            const float l = acc + p.bias[c];
            lg[c] = l;
            if (p.logits_out) p.logits_out[(long long)b * p.C + c] = l;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (wave != 0) return;
    float m = -INFINITY, s = 0.f, v = -INFINITY;
    int i = 0x7fffffff;
    for (int c = lane; c < p.C; c += 64) {
        const float l = lg[c];
        if (l > v || (l == v && c < i) || i == 0x7fffffff) { v = l; i = c; }
        const float mn = fmaxf(m, l);
        s = (m == -INFINITY ? 0.f : s * expf(m - mn)) + expf(l - mn);
        m = mn;
    }
    probe_wave_softmax_argmax(m, s, v, i);
    const float lse = m + logf(s);
    for (int c = lane; c < p.C; c += 64) p.log_probs[(long long)b * p.C + c] = lg[c] - lse;
    if (lane == 0) p.pred[b] = i == 0x7fffffff ? 0 : (long long)i;
}

}  // namespace ac
