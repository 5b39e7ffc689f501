// Bidirectional, length-aware LSTM recurrence of the TokenProbe (probe_path.hip): torch.nn.LSTM(bidirectional=True)
// on packed sequences, zero initial state, gate order i, f, g, o.
//
// The input projections of both directions of a layer for ALL frames are one linear_rows call written as gin[b][t][dir][4H] (bias b_ih +
// b_hh folded).  What is left is sequential in the step s, and follows lstm_step_kernel (lstm.h): one plain launch per step, workgroup =
// 32 clips x 4 hidden units (16 gate columns), 4 waves = 2 clip sub-tiles x 2 K-halves on v_mfma_f32_16x16x4_f32, W_hh pre-packed in
// B-fragment order, h kept in A-fragment order and ping-ponged between two buffers, every load of the step issued before the first MFMA,
// the K-halves meeting in LDS, 128 threads finishing the cell.  blockIdx.z is the direction.  Clip b of length L_b (clamped into 0..N
// here, on the device):
//     forward   handles frame t = s            while s < L_b
//     backward  handles frame t = L_b - 1 - s  while s < L_b      -- it starts at the clip's own last valid frame
// A clip past its length writes nothing -- not y, not c, not h: its rows of the ping-pong buffers go stale, which nobody reads, because a
// row of the MFMA's A operand only reaches the same row of its result and a clip that stopped never resumes.  y is row-major
// y[b][t][dir * H + u] in a buffer the chain zeroed before step 0, so frames beyond a length stay exactly zero (pad_packed_sequence).
// No workgroup waits for another and nothing is counted: the order of the steps is the order of the launches.
#pragma once
#include <hip/hip_runtime.h>
#include "lstm.h"

namespace ac {

struct BiLstmStep {
    const float* gin;          // [B][N][2][4H]
    const float* wpk;          // [2 dirs][H/4 unit groups][H/16 k-steps][64 lanes][4]: W_hh of each direction in B-fragment order
    const float* hprev;        // [2 dirs][Bpad/16][H/16][64][4]: h of step s - 1 in A-fragment order (hfrag_index); not read at s = 0
    float* hnext;              // the same layout: h of step s
    float* c;                  // [2 dirs][Bpad][H]
    float* y;                  // [B][N][2H]
    const long long* lengths;  // [B] absolute frame counts or null (all N)
    int B, Bpad, N, s;
};

__device__ __forceinline__ int probe_len(const long long* lengths, int b, int N) {
    if (!lengths) return N;
    const long long l = lengths[b];
    return l < 0 ? 0 : (l > N ? N : (int)l);
}

template <int KS>   // 16-wide k-steps per K-half: H = 32 * KS
__global__ __launch_bounds__(256) void bilstm_step_kernel(const BiLstmStep p) {
    __shared__ float red[2][2][16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int msub = wave & 1, khalf = wave >> 1;
    const int li = lane & 15, kq = lane >> 4;
    const int ug = blockIdx.x;
    const int b0 = blockIdx.y * 32;
    const int dir = blockIdx.z;
    constexpr int H = 32 * KS;
    const bool first = p.s == 0;
    const long long dstate = (long long)dir * p.Bpad * H;       // this direction's h (either buffer) and c

    // ---- epilogue operands first (128 threads: clip bl, unit ul), so their latency hides under the MFMAs
    const int bl = tid >> 2, ul = tid & 3;
    const int eb = b0 + bl, eu = ug * 4 + ul;
    bool ethread = tid < 128 && eb < p.B;
    int t = 0;
    if (ethread) {
        const int L = probe_len(p.lengths, eb, p.N);
        ethread = p.s < L;
        t = dir == 0 ? p.s : L - 1 - p.s;
    }
    float gpre[4] = {0.f, 0.f, 0.f, 0.f}, cprev = 0.f;
    if (ethread) {
        const float* g = p.gin + (((long long)eb * p.N + t) * 2 + dir) * (4 * H);
#pragma unroll
        for (int q = 0; q < 4; ++q) gpre[q] = g[q * H + eu];
        if (!first) cprev = p.c[dstate + (long long)eb * H + eu];
    }

    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    if (!first) {
        const float* hrow = p.hprev + dstate + (((long long)((b0 >> 4) + msub) * (H / 16) + (long long)khalf * KS) * 64 + lane) * 4;
        const float* wrow = p.wpk + (long long)dir * 4 * H * H + ((long long)ug * (H / 16) + (long long)khalf * KS) * 256 + lane * 4;
        f32x4 a[KS], w[KS];
#pragma unroll
        for (int i = 0; i < KS; ++i) {
            a[i] = *reinterpret_cast<const f32x4*>(hrow + (long long)i * 256);
            w[i] = *reinterpret_cast<const f32x4*>(wrow + (long long)i * 256);
        }
        // keep ALL loads of the step in flight before the first MFMA (lstm.h)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < KS; ++i) {
#pragma unroll
            for (int u = 0; u < 4; u += 2) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][u], w[i][u], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][u + 1], w[i][u + 1], acc1, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[khalf][msub][kq * 4 + r][li] = acc0[r] + acc1[r];
    __syncthreads();
    if (ethread) {
        const int ms = bl >> 4, row = bl & 15;
        float pre[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pre[q] = gpre[q] + (red[0][ms][row][q * 4 + ul] + red[1][ms][row][q * 4 + ul]);
        const float ig = sigmoidf_(pre[0]), fg = sigmoidf_(pre[1]), gg = tanhf_(pre[2]), og = sigmoidf_(pre[3]);
        const float cn = fg * cprev + ig * gg;
        const float hn = og * tanhf_(cn);
        p.c[dstate + (long long)eb * H + eu] = cn;
        p.hnext[dstate + hfrag_index(eb, eu, H)] = hn;
        p.y[((long long)eb * p.N + t) * (2 * H) + dir * H + eu] = hn;
    }
}

}  // namespace ac
