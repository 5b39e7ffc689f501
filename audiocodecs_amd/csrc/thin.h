// HBM-bound ends of the SEANet stack, where one side of the layer has 1 channel and a GEMM tile would
// be almost empty:
//   stem_kernel : [HF] EncodecEncoder.layers[0]  Conv1d(1, F, k)  sig[B][T] -> x[B][T][F] (raw and ELU'd)
//   head_kernel : [HF] EncodecDecoder.layers[-1] Conv1d(F, 1, k)  ELU'd y[B][T][F] -> sig[B][T]
// Both are causal with reflect padding ([HF] modeling_encodec.py:157-176, small-input rule :148-155) or, for
// Mimi's SEANet, zero padding; the stem also applies the length mask (audiocodecs/encodec.py:84-92, [HF]:589-590).
// Algorithmic bytes: stem 4*T*(1 + F*flavours), head 4*T*(F + 1) per clip; plain fp32 FMAs (the
// arithmetic is ~1 flop/B).  Accumulation order: bias first, then taps (and channels) ascending.
#pragma once
#include <hip/hip_runtime.h>
#include "tap_gemm.h"
#include "split16.h"

namespace ac {

struct ThinParams {
    const float* x;        // stem: [B][T]; head: [B][T][F]
    const float* w;        // stem: [F][k] (HF layout [F][1][k]); head: [k][F] (re-packed from [1][F][k])
    const float* bias;     // stem: [F]; head: [1]
    const float* rel_len;  // stem only, optional [B]
    float* y;              // stem: raw [B][T][F] (may be null); head: [B][T]
    float* y_elu;          // stem: ELU'd [B][T][F] (may be null)
    int B, T, F, k;
    int Lp;                // reflect base length: T if T > k-1 else k ([HF]:148-155)
    int pad;               // PAD_REFLECT (EnCodec) or PAD_ZERO (Mimi: pad_mode "constant", [HF] mimi :336-338)
    int padl;              // left padding in samples: k-1 (causal) or (k-1)/2 (DAC, symmetric zero padding)
    const float* alpha;    // stem: Snake parameters of the consumer -> y_elu = snake(y) instead of ELU(y) (DAC)
    const float* alpha_inv;
    int tanh_out;          // head: tanh on the output (DAC decoder, [HF] dac :439-440)
    unsigned* amax_out;    // stem: optional split16.h amax slot [B] of the output (raw and activated flavour)
};

__device__ __forceinline__ int reflect_src(int i, int T, int Lp, int pad) {
    int j = i;
    if (pad == PAD_REFLECT) j = i < 0 ? -i : (i >= Lp ? 2 * (Lp - 1) - i : i);
    return (j >= 0 && j < T) ? j : -1;
}

constexpr int STEM_TT = 2048;   // time steps per workgroup

// F must be a multiple of 4 (<= 128): thread = (time step, 4 channels); k <= 8.
__global__ __launch_bounds__(256) void stem_kernel(const ThinParams p) {
    __shared__ float xs[STEM_TT + THIN_MAXK];
    const int b = blockIdx.y, t0 = blockIdx.x * STEM_TT, tid = threadIdx.x;
    const float* xb = p.x + (long long)b * p.T;
    float alen = 3.0e38f;
    if (p.rel_len) alen = (float)p.T * p.rel_len[b];
    const int pad = p.k - 1;
    for (int e = tid; e < STEM_TT + pad; e += 256) {
        const int j = reflect_src(t0 - p.padl + e, p.T, p.Lp, p.pad);
        xs[e] = (j >= 0 && (float)j < alen) ? xb[j] : 0.f;
    }
    const int cq = p.F / 4;                 // float4 groups per time step
    const int c4 = (tid % cq) * 4;
    float w[4][THIN_MAXK], bv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        bv[c] = p.bias[c4 + c];
#pragma unroll
        for (int j = 0; j < THIN_MAXK; ++j) w[c][j] = j < p.k ? p.w[(c4 + c) * p.k + j] : 0.f;
    }
    __syncthreads();
    const int tstep = 256 / cq;
    const long long ob = (long long)b * p.T * p.F;
    unsigned omax = 0;
    for (int tl = tid / cq; tl < STEM_TT; tl += tstep) {
        const int t = t0 + tl;
        if (t >= p.T) break;
        f32x4 acc = f32x4{bv[0], bv[1], bv[2], bv[3]};
#pragma unroll
        for (int j = 0; j < THIN_MAXK; ++j) {
            if (j < p.k) {
                const float xv = xs[tl + j];
                acc.x = fmaf(w[0][j], xv, acc.x); acc.y = fmaf(w[1][j], xv, acc.y);
                acc.z = fmaf(w[2][j], xv, acc.z); acc.w = fmaf(w[3][j], xv, acc.w);
            }
        }
        const long long o = ob + (long long)t * p.F + c4;
        amax_acc4(omax, acc);
        if (p.y) *reinterpret_cast<f32x4*>(p.y + o) = acc;
        if (p.y_elu) {
            f32x4 w;
            if (p.alpha) {
                const f32x4 al = *reinterpret_cast<const f32x4*>(p.alpha + c4), ai = *reinterpret_cast<const f32x4*>(p.alpha_inv + c4);
                w.x = snake1(acc.x, al.x, ai.x); w.y = snake1(acc.y, al.y, ai.y); w.z = snake1(acc.z, al.z, ai.z); w.w = snake1(acc.w, al.w, ai.w);
                amax_acc4(omax, w);                  // Snake can exceed |acc| (ELU cannot)
            } else {
                w = elu4(acc);
            }
            *reinterpret_cast<f32x4*>(p.y_elu + o) = w;
        }
    }
    if (p.amax_out) amax_flush(omax, amax_at(p.amax_out, b));
}

constexpr int HEAD_TT = 256;    // outputs per workgroup (one per thread)

// F multiple of 4, F <= 128, k <= 8.  LDS: (HEAD_TT + k - 1) rows of F (+4 pad) floats + the weights.
__global__ __launch_bounds__(256) void head_kernel(const ThinParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, FP = F + 4;
    float* xs = smem;                                   // [(HEAD_TT + pad)][FP]
    float* ws = smem + (HEAD_TT + THIN_MAXK) * FP;      // [k][F]
    const int b = blockIdx.y, t0 = blockIdx.x * HEAD_TT, tid = threadIdx.x;
    const int pad = p.k - 1, fq = F / 4;
    const float* xb = p.x + (long long)b * p.T * F;
    for (int e = tid; e < (HEAD_TT + pad) * fq; e += 256) {
        const int row = e / fq, q = e % fq;
        const int j = reflect_src(t0 - p.padl + row, p.T, p.Lp, p.pad);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j >= 0) v = *reinterpret_cast<const f32x4*>(xb + (long long)j * F + 4 * q);
        *reinterpret_cast<f32x4*>(&xs[row * FP + 4 * q]) = v;
    }
    for (int e = tid; e < p.k * F; e += 256) ws[e] = p.w[e];
    __syncthreads();
    const int t = t0 + tid;
    if (t >= p.T) return;
    float acc = p.bias[0];
    for (int j = 0; j < p.k; ++j) {
        const float* xr = &xs[(tid + j) * FP];
        const float* wr = &ws[j * F];
        for (int q = 0; q < fq; ++q) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + 4 * q);
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + 4 * q);
            acc = fmaf(wv.x, xv.x, acc); acc = fmaf(wv.y, xv.y, acc);
            acc = fmaf(wv.z, xv.z, acc); acc = fmaf(wv.w, xv.w, acc);
        }
    }
    p.y[(long long)b * p.T + t] = p.tanh_out ? tanhf(acc) : acc;
}

// head4_kernel (round 4): the same layer for F % 16 == 0 with FOUR lanes per output sample, each over a quarter of the channels
// (all taps), the quarters added pairwise ((q0 + q1) + (q2 + q3)), the bias last.  head_kernel walks a sample's k F products as
// ONE sequential fp32 chain per thread behind a 256-row staging tile: two workgroups per CU, 448 dependent FMAs per thread for
// Mimi's 64 channels -- 2.7 TB/s on a layer that only reads (Mimi 128 x 10 s: 2.9 ms; DAC: 3 % of its step).  Here a workgroup
// stages 64 + k - 1 rows (21 KB: seven workgroups per CU), a thread's chain is k F / 4 long; LDS pitch F + 4 floats: the 16 lanes
// of a 16-byte read group (4 samples x 4 quarters) cover all 64 banks.  The summation ORDER differs from head_kernel's (fp32
// rounding only; both are within the parity tolerance of the waveform, tests/test_*_gpu_parity.py).
constexpr int HEAD4_TT = 64;    // outputs per workgroup

__global__ __launch_bounds__(256) void head4_kernel(const ThinParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int F = p.F, FP = F + 4;
    float* xs = smem;                                    // [(HEAD4_TT + pad)][FP]
    float* ws = smem + (HEAD4_TT + THIN_MAXK) * FP;      // [k][F]
    const int b = blockIdx.y, t0 = blockIdx.x * HEAD4_TT, tid = threadIdx.x;
    const int pad = p.k - 1, fq = F / 4, fqq = fq / 4;
    const float* xb = p.x + (long long)b * p.T * F;
    for (int e = tid; e < (HEAD4_TT + pad) * fq; e += 256) {
        const int row = e / fq, q = e % fq;
        const int j = reflect_src(t0 - p.padl + row, p.T, p.Lp, p.pad);
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (j >= 0) v = *reinterpret_cast<const f32x4*>(xb + (long long)j * F + 4 * q);
        *reinterpret_cast<f32x4*>(&xs[row * FP + 4 * q]) = v;
    }
    for (int e = tid; e < p.k * F; e += 256) ws[e] = p.w[e];
    __syncthreads();
    const int tl = tid >> 2, q = tid & 3;                // four adjacent lanes share a sample
    float acc = 0.f;
    for (int j = 0; j < p.k; ++j) {
        const float* xr = &xs[(tl + j) * FP + q * fqq * 4];
        const float* wr = &ws[j * F + q * fqq * 4];
        for (int g = 0; g < fqq; ++g) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(xr + 4 * g);
            const f32x4 wv = *reinterpret_cast<const f32x4*>(wr + 4 * g);
            acc = fmaf(wv.x, xv.x, acc); acc = fmaf(wv.y, xv.y, acc);
            acc = fmaf(wv.z, xv.z, acc); acc = fmaf(wv.w, xv.w, acc);
        }
    }
    acc += __shfl_xor(acc, 1);                           // q0 + q1 | q2 + q3
    acc += __shfl_xor(acc, 2);                           // (q0 + q1) + (q2 + q3): the same value in the four lanes (fp32 + is commutative)
    const int t = t0 + tl;
    if (q == 0 && t < p.T) {
        const float v = acc + p.bias[0];
        p.y[(long long)b * p.T + t] = p.tanh_out ? tanhf(v) : v;
    }
}

// Polyphase windowed-sinc sample-rate conversion: what torchaudio.functional.resample applies at the
// Codec boundary (audiocodecs/codec.py:59-63,95-99): zero-pad (width, width + o), conv1d with the
// [n phases][taps] kernel at stride o, interleave the phases, truncate.  out[i*n + ph] =
// sum_k kern[ph][k] * x[i*o + k - width].  One thread per output sample; HBM-bound (4*(L + L_out) B/clip).
struct ResampleParams {
    const float* x;      // [B][L]
    const float* kern;   // [n][taps]
    float* y;            // [B][L_out]
    int B, L, L_out, n, o, taps, width;
};

__global__ __launch_bounds__(256) void resample_kernel(const ResampleParams p) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (gid >= p.L_out) return;
    const int i = (int)(gid / p.n), ph = (int)(gid % p.n);
    const float* xb = p.x + (long long)b * p.L;
    const float* kr = p.kern + (long long)ph * p.taps;
    const int base = i * p.o - p.width;
    float acc = 0.f;
    for (int k = 0; k < p.taps; ++k) {
        const int m = base + k;
        if (m >= 0 && m < p.L) acc = fmaf(kr[k], xb[m], acc);
    }
    p.y[(long long)b * p.L_out + gid] = acc;
}

// The same conversion, push by push (ac_resample_stream_*).  Output group i (the n outputs i*n .. i*n + n - 1)
// reads the inputs i*o - width .. i*o - width + taps - 1; it is complete once width + o + i*o samples are in, so after `total` samples
// G(total) = total < width + o ? 0 : (total - width - o) / o + 1 groups are, and a push emits the groups G(before) .. G(after) - 1.
// The oldest input a later group still needs lies fewer than taps samples back: the state keeps the last taps - 1 samples per stream
// (zeros before the stream's start).  A closing push takes all later input as zero and emits up to ceil(n * total / o) outputs.
//
// State (device memory of the caller, 256-byte aligned):
//   [0, 256)                        RStreamHeader: written by a reset, read-only afterwards
//   [256, 256 + align256(8 B))      consumed[B]: input samples taken so far per stream, RSTREAM_FINISHED after the closing push
//   [.., + align256(4 B (taps-1)))  hist[B][taps - 1]: the last taps - 1 input samples, oldest first
// A push is two launches: resample_stream_kernel reads hist and the chunk and writes the outputs; resample_stream_hist_kernel, one
// workgroup per stream, then moves hist on (through LDS: a chunk shorter than the history shifts it in place) and advances consumed[b].
// Both check the header and their stream's count against the call's arguments (the only writer of consumed[b] is workgroup b of the
// second launch, so no workgroup reads a word another one writes in the same launch); on a mismatch the first writes NaN to its outputs
// and the second leaves the state as it is.
constexpr unsigned RSTREAM_MAGIC = 0x54535352u;    // "RSST"
constexpr long long RSTREAM_FINISHED = -1;

struct RStreamHeader {
    unsigned magic;
    int B, n, o, taps, width;
};

struct ResampleStreamParams {
    const float* x;          // [B][x_pitch]: L new samples per stream
    const float* kern;       // [n][taps]
    float* y;                // [B][y_pitch]: this push's m outputs per stream
    const RStreamHeader* hdr;
    long long* consumed;     // [B]
    float* hist;             // [B][taps - 1]
    long long before;        // samples consumed before this push (the caller's count)
    long long out0;          // absolute index of this push's first output: n * G(before)
    long long x_pitch, y_pitch;
    int B, L, m, n, o, taps, width, finish;
};

__device__ __forceinline__ bool rstream_state_ok(const ResampleStreamParams& p, int b) {
    const RStreamHeader h = *p.hdr;
    return h.magic == RSTREAM_MAGIC && h.B == p.B && h.n == p.n && h.o == p.o && h.taps == p.taps && h.width == p.width &&
           p.consumed[b] == p.before;
}

// One output of a push: filter row kr [taps] over (hb [taps - 1] ++ xb [L]).  `base` is the position of tap 0 relative to the chunk's first
// sample; >= -(taps - 1) because the output's group was not complete before this push.
__device__ __forceinline__ float rstream_dot(const float* kr, const float* hb, const float* xb, int base, int taps, int L) {
    const int H = taps - 1;
    float acc = 0.f;
    for (int k = 0; k < taps; ++k) {       // ascending k, one fmaf per tap: resample_kernel's chain (a stored zero where it skips)
        const int m = base + k;
        if (m < 0) acc = fmaf(kr[k], hb[H + m], acc);
        else if (m < L) acc = fmaf(kr[k], xb[m], acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void resample_stream_kernel(const ResampleStreamParams p) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (j >= p.m) return;
    float* yb = p.y + (long long)b * p.y_pitch;
    if (!rstream_state_ok(p, b)) {
        yb[j] = __builtin_nanf("");
        return;
    }
    const long long gid = p.out0 + j;
    const long long i = gid / p.n;
    const int ph = (int)(gid % p.n);
    const int H = p.taps - 1;
    yb[j] = rstream_dot(p.kern + (long long)ph * p.taps, p.hist + (long long)b * H, p.x + (long long)b * p.x_pitch,
                        (int)(i * p.o - p.width - p.before), p.taps, p.L);
}

__global__ __launch_bounds__(256) void resample_stream_hist_kernel(const ResampleStreamParams p) {
    extern __shared__ __align__(16) float rs_row[];      // [taps - 1]
    const int b = blockIdx.x;
    if (!rstream_state_ok(p, b)) return;                 // (uniform over the workgroup)
    const int H = p.taps - 1;
    const float* xb = p.x + (long long)b * p.x_pitch;
    float* hb = p.hist + (long long)b * H;
    for (int j = threadIdx.x; j < H; j += 256) {         // new hist[j] = (old hist ++ chunk)[j + L]
        const long long s = (long long)j + p.L;
        rs_row[j] = s < H ? hb[s] : xb[s - H];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < H; j += 256) hb[j] = rs_row[j];
    if (threadIdx.x == 0) p.consumed[b] = p.finish ? RSTREAM_FINISHED : p.before + p.L;
}

__global__ __launch_bounds__(256) void resample_stream_reset_kernel(RStreamHeader* hdr, const RStreamHeader hd, long long* consumed, float* hist) {
    const int b = blockIdx.x;
    float* hb = hist + (long long)b * (hd.taps - 1);
    for (int j = threadIdx.x; j < hd.taps - 1; j += 256) hb[j] = 0.f;
    if (threadIdx.x == 0) {
        consumed[b] = 0;
        if (b == 0) *hdr = hd;
    }
}

// The slot forms (ac_resample_stream_*_slots): the same state, a push of a SUBSET of its streams, each at its own
// phase.  Row r of the push belongs to slot[r] and continues from before[r], that slot's count as the caller holds it; the row derives
// its out0 = n * G(before[r]) and its own length m_r by the rule above, so the rows of one call emit different numbers of samples (the
// grid is sized by the largest, `m`, and no row writes past it).  slot[] and before[] are the caller's device copies: whatever they hold,
// a row whose slot is outside [0, B), whose count is negative or not the state's, or whose header differs, writes NaN to its outputs and
// touches no state, and the kernels index only inside the state and the first m floats of a y row.  Per output the chain is
// resample_stream_kernel's (rstream_dot); the history moves on one workgroup per listed row, and workgroup r is the only writer of
// consumed[slot[r]] and hist[slot[r]] (the host refuses a list that names a slot twice).
struct ResampleSlotsParams {
    const float* x;          // [rows][x_pitch]: L new samples per listed slot
    const float* kern;       // [n][taps]
    float* y;                // [rows][y_pitch]: row r's m_r outputs
    const RStreamHeader* hdr;
    long long* consumed;     // [B]
    float* hist;             // [B][taps - 1]
    const int* slot;         // [rows] (device)
    const long long* before; // [rows] (device): samples slot[r] consumed before this push
    long long x_pitch, y_pitch;
    int rows, B, L, m, n, o, taps, width, finish;
};

__device__ __forceinline__ long long rstream_groups(long long total, int o, int width) {
    return total < (long long)width + o ? 0 : (total - width - o) / o + 1;
}

// row r's slot, or -1 when the row must not touch the state
__device__ __forceinline__ int rslots_row(const ResampleSlotsParams& p, int r, long long before) {
    const RStreamHeader h = *p.hdr;
    const int s = p.slot[r];
    if (h.magic != RSTREAM_MAGIC || h.B != p.B || h.n != p.n || h.o != p.o || h.taps != p.taps || h.width != p.width) return -1;
    if (s < 0 || s >= p.B || before < 0 || before > (1ll << 62) / p.n - p.L) return -1;
    return p.consumed[s] == before ? s : -1;
}

__global__ __launch_bounds__(256) void resample_slots_kernel(const ResampleSlotsParams p) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int r = blockIdx.y;
    if (j >= p.m) return;
    float* yr = p.y + (long long)r * p.y_pitch;
    const long long before = p.before[r];
    long long out0 = 0, m_r = p.m;                       // (a count that is not a count: the row's own length is unknown, all m are NaN)
    if (before >= 0 && before <= (1ll << 62) / p.n - p.L) {
        const long long total = before + p.L;
        out0 = p.n * rstream_groups(before, p.o, p.width);
        m_r = (p.finish ? (p.n * total + p.o - 1) / p.o : p.n * rstream_groups(total, p.o, p.width)) - out0;
    }
    if (j >= m_r) return;                                // behind m_r: left as it is
    const int s = rslots_row(p, r, before);
    if (s < 0) {
        yr[j] = __builtin_nanf("");
        return;
    }
    const long long gid = out0 + j;
    const long long i = gid / p.n;
    const int H = p.taps - 1;
    yr[j] = rstream_dot(p.kern + (gid % p.n) * p.taps, p.hist + (long long)s * H, p.x + (long long)r * p.x_pitch,
                        (int)(i * p.o - p.width - before), p.taps, p.L);
}

__global__ __launch_bounds__(256) void resample_slots_hist_kernel(const ResampleSlotsParams p) {
    extern __shared__ __align__(16) float rs_row[];      // [taps - 1]
    const int r = blockIdx.x;
    const long long before = p.before[r];
    const int s = rslots_row(p, r, before);
    if (s < 0) return;                                   // (uniform over the workgroup)
    const int H = p.taps - 1;
    const float* xr = p.x + (long long)r * p.x_pitch;
    float* hb = p.hist + (long long)s * H;
    for (int j = threadIdx.x; j < H; j += 256) {
        const long long q = (long long)j + p.L;
        rs_row[j] = q < H ? hb[q] : xr[q - H];
    }
    __syncthreads();
    for (int j = threadIdx.x; j < H; j += 256) hb[j] = rs_row[j];
    if (threadIdx.x == 0) p.consumed[s] = p.finish ? RSTREAM_FINISHED : before + p.L;
}

// the listed slots start afresh; the header is compared, never written (one workgroup per row)
__global__ __launch_bounds__(256) void resample_slots_reset_kernel(const RStreamHeader* hdr, const RStreamHeader hd, long long* consumed, float* hist,
                                                                   const int* slot) {
    const RStreamHeader h = *hdr;
    const int s = slot[blockIdx.x];
    if (h.magic != hd.magic || h.B != hd.B || h.n != hd.n || h.o != hd.o || h.taps != hd.taps || h.width != hd.width) return;
    if (s < 0 || s >= hd.B) return;
    float* hb = hist + (long long)s * (hd.taps - 1);
    for (int j = threadIdx.x; j < hd.taps - 1; j += 256) hb[j] = 0.f;
    if (threadIdx.x == 0) consumed[s] = 0;
}

}  // namespace ac
