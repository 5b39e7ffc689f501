// Streaming EnCodec (encodec_stream.hip; DESIGN.md "Streaming EnCodec"): the one kernel the stream adds to the shared staging kernels of
// stream_stage.h -- the LSTM time step that starts from a carried state.
//
// estream_lstm_step_kernel: one launch = one time step of one layer for all B streams.
//   gates[b] = (gin[b] + bias) + W_hh h[t-1][b];  c = f c + i g;  h[t] = o tanh(c)   (gate order i, f, g, o; [HF] EncodecLSTM :236-249)
//   gin is the input projection W_ih x[t] of the whole push, computed before the first step (one skinny product or one tap-GEMM).
// A workgroup owns FOUR hidden units = 16 gate rows of W_hh, read in the order the handle already packs for lstm_step_kernel
// (LstmPlan::hh_off: [unit group][k-step of 16][lane (row j = 4 gate + unit, k quarter kq)][4 fp32]): a wave-instruction covers 1 KiB of it, the
// weights are the launch's only traffic that scales (4 D D fp32 = 4 MB per step and layer at D = 512, every byte read once) and stay in
// registers while the workgroup walks its streams, 64 per workgroup (grid.y chunks the batch).  Its 4 waves split the k-steps (wave w
// takes k-steps w, w + 4, ..); h[t-1] comes from L2 as 16-byte vectors, four streams in flight at a time.
// Summation order of a gate pre-activation: lane (j, kq) of wave w adds, in ascending k-step, the products at k = 16 ks + 4 kq + (0..3) with
// one fmaf each; the four k quarters fold by the xor butterfly 16, 32; the waves add in the order 0 .. 3.  It depends on D alone: a stream's
// result is bit-identical whatever shares the launch.  Exact fp32 products in both precisions; no atomics, no scratch.
// The epilogue (thread = (stream, unit)) applies the non-linearities (lstm.h sigmoidf_ / tanhf_), updates c IN PLACE in the stream state,
// writes h[t] to the push's h sequence (the next step's and the next layer's operand) and, on the push's last step, to the state;
// the last layer also writes ELU(h[t] + x[t]), the module's skip connection in the flavour the following conv reads.
//
// A slot push (ac_encodec_stream_encode_slots / _decode_slots) runs n of the state's streams: every buffer of the push is dense [n], and
// the step kernel reaches the state's c and h rows through the slot map of stream_stage.h (mstream_slot).  Two small kernels go with it:
//   estream_gather_h_kernel     the carried h of the listed streams [L][cap][D] -> the push's dense copy [L][n][D]
//   estream_reset_slots_kernel  position = 0, fresh = 1, h = c = 0 for the listed streams and nothing else
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lstm.h"
#include "tap_gemm.h"
#include "stream_stage.h"

constexpr unsigned ESTREAM_MAGIC = 0x54534345u;   // "ECST"
constexpr unsigned EDSTREAM_MAGIC = 0x54534445u;  // "EDST": a decode state (its own layout; never accepted where an encode state is expected)

struct EStreamLstmParams {
    const float* wpk;            // W_hh of the layer, LstmPlan::hh_off order
    const float* bias;           // [4D] b_ih + b_hh
    const float* gin;            // W_ih x[t] of stream b at gin + b * gin_bs: [4D]
    const float* hprev;          // h[t-1] of stream b at hprev + b * hprev_bs: [D], 16-byte aligned (never the buffer hout / hstate point into)
    float* hout;                 // h[t] of stream b at hout + b * hout_bs
    float* hstate;               // null, or the state's h [B][D] (the push's last step)
    float* c;                    // the state's c [B][D], updated in place
    const float* skip;           // last layer: x[t] of stream b at skip + b * skip_bs (null: not the last layer)
    float* yelu;                 // last layer: ELU(h[t] + x[t]) of stream b at yelu + b * y_bs
    long long gin_bs, hprev_bs, hout_bs, skip_bs, y_bs;
    int B, D;
    const int* slot;             // null, or [B] (device): row b's c and hstate rows are those of stream slot[b] of the `cap` the state holds
    int cap;
};

template <int KPW>   // k-steps per wave: D = 64 * KPW
__global__ __launch_bounds__(256) void estream_lstm_step_kernel(const EStreamLstmParams p) {
    __shared__ float part[4][64][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kq = lane >> 4;
    const int ug = blockIdx.x, b0 = blockIdx.y * 64;
    const int nb = p.B - b0 < 64 ? p.B - b0 : 64;
    const int D = p.D;
    // the epilogue's operands first: their latency hides behind the products
    const int ebl = tid >> 2, eu = tid & 3, unit = ug * 4 + eu;
    const bool live = ebl < nb;
    const long long eb = b0 + (live ? ebl : 0);
    float gi[4], c_old, sk = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g) gi[g] = __fadd_rn(p.gin[eb * p.gin_bs + g * D + unit], p.bias[g * D + unit]);
    const long long es = mstream_slot(p.slot, (int)eb, p.cap);       // the row of the state's c and h (-1: none, the row touches no state)
    c_old = es >= 0 ? p.c[es * D + unit] : 0.f;
    if (p.skip) sk = p.skip[eb * p.skip_bs + unit];

    ac::f32x4 w[KPW];
    const ac::f32x4* wp = reinterpret_cast<const ac::f32x4*>(p.wpk) + (long long)ug * (D / 16) * 64 + lane;
#pragma unroll
    for (int i = 0; i < KPW; ++i) w[i] = wp[(long long)(wave + 4 * i) * 64];
    for (int bl0 = 0; bl0 < nb; bl0 += 4) {
        ac::f32x4 hv[4][KPW];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int bl = bl0 + q < nb ? bl0 + q : nb - 1;          // streams past the end repeat the last one; their sums are not stored
            const float* hr = p.hprev + (long long)(b0 + bl) * p.hprev_bs + 4 * kq;
#pragma unroll
            for (int i = 0; i < KPW; ++i) hv[q][i] = *reinterpret_cast<const ac::f32x4*>(hr + (wave + 4 * i) * 16);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < KPW; ++i) {
                acc = fmaf(w[i].x, hv[q][i].x, acc);
                acc = fmaf(w[i].y, hv[q][i].y, acc);
                acc = fmaf(w[i].z, hv[q][i].z, acc);
                acc = fmaf(w[i].w, hv[q][i].w, acc);
            }
            acc = __fadd_rn(acc, __shfl_xor(acc, 16));
            acc = __fadd_rn(acc, __shfl_xor(acc, 32));
            if (lane < 16 && bl0 + q < nb) part[wave][bl0 + q][lane] = acc;
        }
    }
    __syncthreads();
    if (!live) return;
    float pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int j = g * 4 + eu;
        const float rec = __fadd_rn(__fadd_rn(__fadd_rn(part[0][ebl][j], part[1][ebl][j]), part[2][ebl][j]), part[3][ebl][j]);
        pre[g] = __fadd_rn(gi[g], rec);
    }
    const float ig = ac::sigmoidf_(pre[0]), fg = ac::sigmoidf_(pre[1]), gg = ac::tanhf_(pre[2]), og = ac::sigmoidf_(pre[3]);
    const float cn = __fadd_rn(__fmul_rn(fg, c_old), __fmul_rn(ig, gg));
    const float hn = __fmul_rn(og, ac::tanhf_(cn));
    if (es >= 0) p.c[es * D + unit] = cn;
    p.hout[eb * p.hout_bs + unit] = hn;
    if (p.hstate && es >= 0) p.hstate[es * D + unit] = hn;
    if (p.skip) p.yelu[eb * p.y_bs + unit] = ac::elu1(__fadd_rn(hn, sk));
}

// dst [L][n][D] = hstate [L][cap][D] rows slot[0 .. n): the dense copy of the carried h that step 0 of a slot push reads (the lockstep
// push takes it with one memcpy).  One thread per 16 bytes; a row whose map entry is outside [0, cap) reads nothing and gets zeros.
template <int U = 0>
__global__ __launch_bounds__(256) void estream_gather_h_kernel(const float* hstate, float* dst, const int* slot, int n, int cap, int L, int D) {
    const int D4 = D / 4;
    const long long total = (long long)L * n * D4;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int d = (int)(e % D4);
        const long long lb = e / D4;
        const int b = (int)(lb % n), l = (int)(lb / n);
        const int sb = mstream_slot(slot, b, cap);
        ac::f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (sb >= 0) v = reinterpret_cast<const ac::f32x4*>(hstate + ((long long)l * cap + sb) * D)[d];
        reinterpret_cast<ac::f32x4*>(dst + ((long long)l * n + b) * D)[d] = v;
    }
}

// One workgroup per listed stream: position = 0, fresh = 1, and the stream's h and c rows of every layer = 0.  Nothing else is touched
// (not the header, not the conv histories: a fresh stream's are rebuilt from its first push); an entry outside [0, cap) is skipped.
template <int U = 0>
__global__ __launch_bounds__(256) void estream_reset_slots_kernel(long long* pos, int* fresh, float* hstate, float* cstate, const int* slot, int n, int cap,
                                                                  int L, int D) {
    const int b = blockIdx.x;
    if (b >= n) return;
    const int sb = mstream_slot(slot, b, cap);
    if (sb < 0) return;
    if (threadIdx.x == 0) {
        pos[sb] = 0;
        fresh[sb] = 1;
    }
    for (int e = threadIdx.x; e < L * D; e += 256) {
        const long long o = ((long long)(e / D) * cap + sb) * D + e % D;
        hstate[o] = 0.f;
        cstate[o] = 0.f;
    }
}
