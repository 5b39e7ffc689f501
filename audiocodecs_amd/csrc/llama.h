// llama.h: the kernels of the Llama decoder with a KV cache (lm_path.hip).  Plain launches only: no kernel waits
// for another workgroup, counts arrivals or is launched cooperatively.  Everything that depends on the position is read from the state's
// header words on the device, so a captured step replays without new arguments.
//
//   * rows: a launch works on the rows (b, i), b < B, i = i0 + j * istep, j < T, of a call over Tfull rows per batch entry; row (b, i)
//     of a dense buffer is its row b * Tfull + i and sits at position cur + i of the cache (cur: header word LMH_CUR).  A step is
//     T = Tfull = 1; the output heads of a forward over many rows take the rows of one codebook each (istep = num_codebooks).
//   * lm_gemv_kernel: y[r][n] = sum_k x[r][k] W[n][k] in fp32 FMAs, a wave per PAIR of weight rows, RT rows per pass with the weights
//     of the pass in registers.  A lane reads float4s of the row, so a wave reads the whole input row anyway: with a norm weight it also
//     sums x^2 and scales the dot products by rsqrt(mean + eps) -- each wave recomputes the row norms it needs, no normalised tensor exists.
//     The pair is what the epilogues need: the (2i, 2i+1) columns that RoPE rotates, column n of w1 with column n of w3.
//     Both this kernel and the attention are bound by trips to memory, not by work: the k loop is unrolled and the attention takes
//     LM_KB keys per trip so that several requests are in flight per wave; the RT sums per lane are reduced by halving (lm_wave_sums).
//   * lm_attn_kernel: one query row, one key/value head, one split of LM_KS keys per workgroup; a wave reads a key row once for all the
//     query heads of the group and keeps (m, l, acc) per head; the four waves meet in LDS; the output is (m, l, acc) per split.
//     lm_attn_combine_kernel merges the splits that hold keys.  No score tensor and no repeated K/V is written.
//   * lm_step_begin_kernel (one workgroup) is the whole bookkeeping of a generated token: hyp, alive, lens, the logits log, the next
//     input's embedding, and the header words -- the ONLY writer of the position.  A step whose position would pass the capacity writes
//     nothing, raises LMH_FLAG and clears LMH_ACTIVE; every other kernel returns at once while LMH_ACTIVE is 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ac {

constexpr int LM_MAX_ROWS = 64;      // rows (batch entries) per state
constexpr int LM_KS = 128;           // keys per attention split
constexpr int LM_KB = 4;             // keys of a wave whose rows are in flight together
constexpr int LM_MAX_HD = 256;       // head dim limit (4 elements per lane)
constexpr int LM_MAX_GROUP = 8;      // query heads per key/value head
constexpr int LM_HDR_WORDS = 64;
// header words of a state (int32); LMH_OFF is an int64 (words 10, 11): the draw offset of the next step's first row
enum { LMH_POS = 0, LMH_CUR = 1, LMH_STEP = 2, LMH_ACTIVE = 3, LMH_FLAG = 4, LMH_B = 5, LMH_CAP = 6, LMH_MAXSTEPS = 7, LMH_OFF = 10 };

struct LmRows {
    int B, T, i0, istep, Tfull;
};

__device__ __forceinline__ void lm_row(const LmRows& r, int m, int& b, int& i) {
    b = m / r.T;
    i = r.i0 + (m - b * r.T) * r.istep;
}

__device__ __forceinline__ float lm_wave_sum(float x) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) x += __shfl_xor(x, sh);
    return x;
}

// The sums of N values per lane (N a power of two <= 64) over the 64 lanes in N - 1 + (6 - log2 N) exchanges instead of 6 N: at the
// exchange over distance 32 >> s a lane keeps one half of what it holds and hands the other half to its partner.  Afterwards v[0] is the
// total of index lm_sum_index<N>(lane) (every lane that shares the top log2 N bits holds the same one).
template <int N>
__device__ __forceinline__ void lm_wave_sums(float (&v)[N], int lane) {
    int off = 32;
#pragma unroll
    for (int n = N; n > 1; n >>= 1, off >>= 1) {
        const bool upper = (lane & off) != 0;
#pragma unroll
        for (int j = 0; j < n / 2; ++j) {
            const float keep = upper ? v[j + n / 2] : v[j], send = upper ? v[j] : v[j + n / 2];
            v[j] = keep + __shfl_xor(send, off);
        }
    }
#pragma unroll
    for (; off > 0; off >>= 1) v[0] += __shfl_xor(v[0], off);
}

template <int N>
__device__ __forceinline__ int lm_sum_index(int lane) {
    int j = 0, bit = 5;
#pragma unroll
    for (int n = N; n > 1; n >>= 1, --bit) j += ((lane >> bit) & 1) * (n / 2);
    return j;
}

enum { LM_EPI_QKV = 0, LM_EPI_RES = 1, LM_EPI_SWIGLU = 2, LM_EPI_HEAD = 3, LM_EPI_PLAIN = 4 };

struct LmGemv {
    const int* hdr;          // null (PLAIN): no state, always runs
    const float* x;          // [B * Tfull][K]
    const float* nw;         // [K] RMSNorm weight or null
    const float* wa;         // weight rows; SWIGLU: w1
    const float* wb;         // SWIGLU: w3
    int K, N, pairs;         // N output columns; pairs = N (SWIGLU) or ceil(N / 2)
    float eps;
    LmRows r;
    float* out;              // RES: the residual stream, updated in place; QKV: q [B * Tfull][nq]; SWIGLU: [B * Tfull][N]; HEAD / PLAIN: row b * out_T + i - out_ioff
    int out_T, out_ioff;
    // QKV
    float* kc;               // [B][cap][nkv][hd]
    float* vc;
    const float* rcos;       // [rows][hd / 2]
    const float* rsin;
    int cap, nq, nkvd, hd;
    int heads;               // HEAD: output heads; the launch's rows use head (cur + i0) % heads
};

template <int EPI, int RT>
__global__ __launch_bounds__(256) void lm_gemv_kernel(const LmGemv p) {
    int cur = 0;
    if constexpr (EPI != LM_EPI_PLAIN) {
        if (!p.hdr[LMH_ACTIVE]) return;
        cur = p.hdr[LMH_CUR];
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pair = blockIdx.x * 4 + wave;
    if (pair >= p.pairs) return;
    const int K = p.K;
    const float *wa, *wb;
    bool has_b = true;
    if constexpr (EPI == LM_EPI_SWIGLU) {
        wa = p.wa + (size_t)pair * K;
        wb = p.wb + (size_t)pair * K;
    } else {
        const float* base = p.wa;
        if constexpr (EPI == LM_EPI_HEAD) base += (size_t)((cur + p.r.i0) % p.heads) * p.N * K;
        wa = base + (size_t)(2 * pair) * K;
        has_b = 2 * pair + 1 < p.N;
        wb = has_b ? wa + K : wa;
    }
    const bool norm = p.nw != nullptr;
    const int M = p.r.B * p.r.T;
    constexpr int LM_TRIPS = RT <= 2 ? 4 : 2;
    for (int m0 = blockIdx.y * RT; m0 < M; m0 += gridDim.y * RT) {
        float a[RT], c[RT], ss[RT];
        const float* xr[RT];
#pragma unroll
        for (int j = 0; j < RT; ++j) {
            a[j] = c[j] = ss[j] = 0.0f;
            int b, i;
            lm_row(p.r, min(m0 + j, M - 1), b, i);
            xr[j] = p.x + ((size_t)b * p.r.Tfull + i) * K;
        }
        // (unrolled: the loads of several trips are in flight together -- a trip's work is far shorter than a trip to memory)
#pragma unroll LM_TRIPS
        for (int k = lane * 4; k < K; k += 256) {
            float4 va = *reinterpret_cast<const float4*>(wa + k), vb = *reinterpret_cast<const float4*>(wb + k);
            if (norm) {
                const float4 g = *reinterpret_cast<const float4*>(p.nw + k);
                va.x *= g.x; va.y *= g.y; va.z *= g.z; va.w *= g.w;
                vb.x *= g.x; vb.y *= g.y; vb.z *= g.z; vb.w *= g.w;
            }
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                const float4 xv = *reinterpret_cast<const float4*>(xr[j] + k);
                a[j] = fmaf(xv.x, va.x, fmaf(xv.y, va.y, fmaf(xv.z, va.z, fmaf(xv.w, va.w, a[j]))));
                c[j] = fmaf(xv.x, vb.x, fmaf(xv.y, vb.y, fmaf(xv.z, vb.z, fmaf(xv.w, vb.w, c[j]))));
                ss[j] = fmaf(xv.x, xv.x, fmaf(xv.y, xv.y, fmaf(xv.z, xv.z, fmaf(xv.w, xv.w, ss[j]))));
            }
        }
        // a lane ends with the sums of ONE row, lm_sum_index(lane); the first lane of each group of 64 / RT writes it
        lm_wave_sums<RT>(a, lane);
        lm_wave_sums<RT>(c, lane);
        if (norm) lm_wave_sums<RT>(ss, lane);
        float ya = a[0], yc = c[0];
        const float ys = ss[0];
        const int m = m0 + lm_sum_index<RT>(lane);
        if ((lane & (64 / RT - 1)) != 0 || m >= M) continue;
        int b, i;
        lm_row(p.r, m, b, i);
        const size_t row = (size_t)b * p.r.Tfull + i;
        if (norm) {
            const float rs = rsqrtf(ys / (float)K + p.eps);
            ya *= rs;
            yc *= rs;
        }
        if constexpr (EPI == LM_EPI_QKV) {
            const int n0 = 2 * pair, pos = cur + i;
            if (n0 < p.nq + p.nkvd) {      // q or k: rotate the pair by row `pos` of the table
                const int n = n0 < p.nq ? n0 : n0 - p.nq;
                const int d = n % p.hd;
                const float cs = p.rcos[(size_t)pos * (p.hd / 2) + d / 2], sn = p.rsin[(size_t)pos * (p.hd / 2) + d / 2];
                const float r0 = ya * cs - yc * sn, r1 = ya * sn + yc * cs;
                float* dst = n0 < p.nq ? p.out + row * p.nq + n : p.kc + ((size_t)b * p.cap + pos) * p.nkvd + n;
                dst[0] = r0;
                dst[1] = r1;
            } else {
                float* dst = p.vc + ((size_t)b * p.cap + pos) * p.nkvd + (n0 - p.nq - p.nkvd);
                dst[0] = ya;
                dst[1] = yc;
            }
        } else if constexpr (EPI == LM_EPI_RES) {
            float* dst = p.out + row * p.N + 2 * pair;
            dst[0] += ya;
            if (has_b) dst[1] += yc;
        } else if constexpr (EPI == LM_EPI_SWIGLU) {
            p.out[row * p.N + pair] = ya / (1.0f + expf(-ya)) * yc;
        } else {
            float* dst = p.out + ((size_t)b * p.out_T + (i - p.out_ioff)) * p.N + 2 * pair;
            dst[0] = ya;
            if (has_b) dst[1] = yc;
        }
    }
}

struct LmAttn {
    const int* hdr;
    const float* q;      // [B * Tfull][nh * hd], rotated
    const float* kc;     // [B][cap][nkv][hd]
    const float* vc;
    float* part;         // [B * T][nh][S][hd + 2]: m, l, acc
    float* out;          // combine: [B * Tfull][nh * hd]
    LmRows r;
    int cap, nh, nkv, hd, S;
    float scale;
};

// grid (S, nkv, B * T)
template <int G, int DPL>
__global__ __launch_bounds__(256) void lm_attn_kernel(const LmAttn p) {
    __shared__ float sh[4][G][DPL * 64 + 2];
    if (!p.hdr[LMH_ACTIVE]) return;
    const int cur = p.hdr[LMH_CUR];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = blockIdx.z, g = blockIdx.y, s = blockIdx.x;
    int b, i;
    lm_row(p.r, m, b, i);
    const int pos = cur + i, k0 = s * LM_KS;
    if (k0 > pos) return;                           // (the whole workgroup: this split holds no key of the row)
    const int k1 = min(k0 + LM_KS, pos + 1), hd = p.hd;
    float qv[G][DPL], acc[G][DPL], mx[G], l[G];
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        const float* qr = p.q + ((size_t)b * p.r.Tfull + i) * ((size_t)p.nh * hd) + (size_t)(g * G + hh) * hd;
        mx[hh] = -INFINITY;
        l[hh] = 0.0f;
#pragma unroll
        for (int e = 0; e < DPL; ++e) {
            const int d = lane + 64 * e;
            qv[hh][e] = d < hd ? qr[d] : 0.0f;
            acc[hh][e] = 0.0f;
        }
    }
    // LM_KB keys of the wave per trip: their rows are requested together (a key's work is far shorter than a trip to memory); a key
    // past the end re-reads the trip's first row and is skipped
    for (int j0 = k0 + wave; j0 < k1; j0 += 4 * LM_KB) {
        float kv[LM_KB][DPL], vv[LM_KB][DPL];
#pragma unroll
        for (int u = 0; u < LM_KB; ++u) {
            const int j = j0 + 4 * u < k1 ? j0 + 4 * u : j0;
            const size_t at = (((size_t)b * p.cap + j) * p.nkv + g) * hd;
#pragma unroll
            for (int e = 0; e < DPL; ++e) {
                const int d = lane + 64 * e;
                kv[u][e] = d < hd ? p.kc[at + d] : 0.0f;
                vv[u][e] = d < hd ? p.vc[at + d] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < LM_KB; ++u) {
            if (j0 + 4 * u >= k1) break;                                    // (the whole wave)
#pragma unroll
            for (int hh = 0; hh < G; ++hh) {
                float sc = 0.0f;
#pragma unroll
                for (int e = 0; e < DPL; ++e) sc = fmaf(qv[hh][e], kv[u][e], sc);
                sc = lm_wave_sum(sc) * p.scale;
                const float mn = fmaxf(mx[hh], sc);
                const float cf = expf(mx[hh] - mn), w = expf(sc - mn);      // (the first key: exp(-inf) = 0)
                l[hh] = l[hh] * cf + w;
#pragma unroll
                for (int e = 0; e < DPL; ++e) acc[hh][e] = fmaf(w, vv[u][e], acc[hh][e] * cf);
                mx[hh] = mn;
            }
        }
    }
#pragma unroll
    for (int hh = 0; hh < G; ++hh) {
        if (lane == 0) {
            sh[wave][hh][DPL * 64] = mx[hh];
            sh[wave][hh][DPL * 64 + 1] = l[hh];
        }
#pragma unroll
        for (int e = 0; e < DPL; ++e) sh[wave][hh][lane + 64 * e] = acc[hh][e];
    }
    __syncthreads();
    for (int hh = wave; hh < G; hh += 4) {          // the waves in order: a wave without a key has m = -inf, weight 0
        float M = -INFINITY;
        for (int w = 0; w < 4; ++w) M = fmaxf(M, sh[w][hh][DPL * 64]);
        float L = 0.0f, o[DPL];
#pragma unroll
        for (int e = 0; e < DPL; ++e) o[e] = 0.0f;
        for (int w = 0; w < 4; ++w) {
            const float f = expf(sh[w][hh][DPL * 64] - M);
            L = fmaf(sh[w][hh][DPL * 64 + 1], f, L);
#pragma unroll
            for (int e = 0; e < DPL; ++e) o[e] = fmaf(sh[w][hh][lane + 64 * e], f, o[e]);
        }
        float* dst = p.part + (((size_t)m * p.nh + (g * G + hh)) * p.S + s) * (hd + 2);
        if (lane == 0) {
            dst[0] = M;
            dst[1] = L;
        }
#pragma unroll
        for (int e = 0; e < DPL; ++e) {
            const int d = lane + 64 * e;
            if (d < hd) dst[2 + d] = o[e];
        }
    }
}

// grid (nh, B * T), 64 threads
template <int DPL>
__global__ __launch_bounds__(64) void lm_attn_combine_kernel(const LmAttn p) {
    if (!p.hdr[LMH_ACTIVE]) return;
    const int cur = p.hdr[LMH_CUR], lane = threadIdx.x, h = blockIdx.x, m = blockIdx.y, hd = p.hd;
    int b, i;
    lm_row(p.r, m, b, i);
    const int ns = (cur + i) / LM_KS + 1;           // the splits that hold keys of this row (<= S: cur + i < cap)
    const float* src = p.part + ((size_t)m * p.nh + h) * p.S * (hd + 2);
    float M = -INFINITY;
    for (int s = 0; s < ns; ++s) M = fmaxf(M, src[(size_t)s * (hd + 2)]);
    float L = 0.0f, o[DPL];
#pragma unroll
    for (int e = 0; e < DPL; ++e) o[e] = 0.0f;
    for (int s = 0; s < ns; ++s) {
        const float* ps = src + (size_t)s * (hd + 2);
        const float f = expf(ps[0] - M);
        L = fmaf(ps[1], f, L);
#pragma unroll
        for (int e = 0; e < DPL; ++e) {
            const int d = lane + 64 * e;
            if (d < hd) o[e] = fmaf(ps[2 + d], f, o[e]);
        }
    }
    float* dst = p.out + ((size_t)b * p.r.Tfull + i) * ((size_t)p.nh * hd) + (size_t)h * hd;
#pragma unroll
    for (int e = 0; e < DPL; ++e) {
        const int d = lane + 64 * e;
        if (d < hd) dst[d] = o[e] / L;
    }
}

// ---- the state's header --------------------------------------------------------------------------------------------------------------

struct LmInit {
    int* hdr;
    int* alive;
    int* lens;
    int B, cap, max_steps;
    long long offset;
};

__global__ __launch_bounds__(64) void lm_reset_kernel(const LmInit p) {
    const int t = threadIdx.x;
    p.hdr[t] = 0;                                   // (LM_HDR_WORDS = 64 = the workgroup)
    p.alive[t] = t < p.B ? 1 : 0;
    p.lens[t] = 0;
    __syncthreads();
    if (t == 0) {
        p.hdr[LMH_B] = p.B;
        p.hdr[LMH_CAP] = p.cap;
        p.hdr[LMH_MAXSTEPS] = p.max_steps;
        *reinterpret_cast<long long*>(p.hdr + LMH_OFF) = p.offset;
    }
}

// a forward over T rows: they go to the positions pos .. pos + T - 1.  The host's position has to be the state's.
__global__ void lm_begin_rows_kernel(int* hdr, int host_pos, int T, int B, int cap) {
    const int pos = hdr[LMH_POS];
    const bool ok = !hdr[LMH_FLAG] && pos == host_pos && hdr[LMH_B] == B && hdr[LMH_CAP] == cap && pos + T <= cap;
    hdr[LMH_ACTIVE] = ok ? 1 : 0;
    if (ok) {
        hdr[LMH_CUR] = pos;
        hdr[LMH_POS] = pos + T;
    } else {
        hdr[LMH_FLAG] = 1;
    }
}

struct LmStep {
    int* hdr;
    int* alive;
    int* lens;
    const long long* tok;    // [B]: the sampler's draw from the pending logits
    long long* hyp;          // [B][max_steps]
    const float* pend;       // [B][C]
    float* log;              // [max_steps][B][C] or null
    const float* emb;        // [num_codebooks * vocab][dim]
    float* x;                // [B][dim]: the next input
    int B, C, vocab, ncb, dim, cap, max_steps;
    long long eos;
};

// One workgroup.  The token of step s is recorded while s < max_steps and some row was alive before it (the reference's loop leaves
// after the step in which the last row ended); the next row is computed while another step follows and some row is still alive.
__global__ __launch_bounds__(256) void lm_step_begin_kernel(const LmStep p) {
    __shared__ int any_before, any_after;
    const int tid = threadIdx.x;
    const int step = p.hdr[LMH_STEP], pos = p.hdr[LMH_POS], flag = p.hdr[LMH_FLAG];
    const bool shape_ok = p.hdr[LMH_B] == p.B && p.hdr[LMH_CAP] == p.cap && p.hdr[LMH_MAXSTEPS] == p.max_steps;
    if (tid == 0) any_before = any_after = 0;
    __syncthreads();
    if (tid < p.B && p.alive[tid]) any_before = 1;
    __syncthreads();
    const bool rec = shape_ok && !flag && step < p.max_steps && any_before;
    if (rec) {
        if (tid < p.B) {
            const long long t = p.tok[tid];
            p.hyp[(size_t)tid * p.max_steps + step] = t;
            const int a = p.alive[tid] && t != p.eos;
            p.alive[tid] = a;
            if (a) {
                p.lens[tid] += 1;
                any_after = 1;
            }
        }
        if (p.log)
            for (int e = tid; e < p.B * p.C; e += 256) p.log[(size_t)step * p.B * p.C + e] = p.pend[e];
    }
    __syncthreads();
    const bool fwd = rec && step + 1 < p.max_steps && any_after;
    const bool active = fwd && pos < p.cap;
    if (active) {
        const int k = (step + 1) % p.ncb;
        for (int e = tid; e < p.B * p.dim; e += 256) {
            const int r = e / p.dim;
            long long t = p.tok[r];
            t = t < 0 ? 0 : t >= p.vocab ? p.vocab - 1 : t;
            p.x[e] = p.emb[((size_t)k * p.vocab + (size_t)t) * p.dim + (e - r * p.dim)];
        }
    }
    if (tid == 0) {
        p.hdr[LMH_ACTIVE] = active ? 1 : 0;
        if ((fwd && !active) || !shape_ok) p.hdr[LMH_FLAG] = 1;
        if (rec) {
            p.hdr[LMH_STEP] = step + 1;
            *reinterpret_cast<long long*>(p.hdr + LMH_OFF) += p.B;
        }
        if (active) {
            p.hdr[LMH_CUR] = pos;
            p.hdr[LMH_POS] = pos + 1;
        }
    }
}

// out[(b * out_T + P + j)][:] = table[tok(b, j) + ((curr_pos + j) % ncb) * vocab][:]
__global__ __launch_bounds__(256) void lm_embed_kernel(const long long* toks, int B, int T, const float* emb, int vocab, int ncb, int dim, int curr_pos,
                                                       float* out, int out_T, int P) {
    const int m = blockIdx.x, b = m / T, j = m - b * T;
    long long t = toks[m];
    t = t < 0 ? 0 : t >= vocab ? vocab - 1 : t;
    const float* src = emb + ((size_t)((curr_pos + j) % ncb) * vocab + (size_t)t) * dim;
    float* dst = out + ((size_t)b * out_T + P + j) * dim;
    for (int d = threadIdx.x; d < dim; d += 256) dst[d] = src[d];
}

// the final norm as a tensor (stages only): one wave per row
__global__ __launch_bounds__(64) void lm_rmsnorm_kernel(const int* hdr, const float* x, const float* w, int dim, float eps, float* out) {
    if (!hdr[LMH_ACTIVE]) return;
    const float* xr = x + (size_t)blockIdx.x * dim;
    float ss = 0.0f;
    for (int d = threadIdx.x; d < dim; d += 64) ss = fmaf(xr[d], xr[d], ss);
    const float rs = rsqrtf(lm_wave_sum(ss) / (float)dim + eps);
    for (int d = threadIdx.x; d < dim; d += 64) out[(size_t)blockIdx.x * dim + d] = xr[d] * rs * w[d];
}

}  // namespace ac
