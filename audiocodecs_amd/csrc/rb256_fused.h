// rb256_fused: EnCodec's 256-channel residual block (EncodecResnetBlock at C = 256, hidden 128, kernel 3, causal reflect padding) as
// ONE kernel that reads the producer's RAW rows.  Unfused the block is two tap_gemm6 launches (k3 conv <1,4,4,1>, [1x1 | shortcut]
// <1,4,4,2>) with the hidden activation in HBM between them and an ELU'd second flavour of the input written by the producer.
// The weights (786 KB as fp16 planes) fit no CU, so this kernel is the two tap_gemm6 main loops run back to back on one 128-row tile
// with all 256 output columns, weight fragments L2 -> registers as there (tap_gemm6.h), the hidden tile handed over through LDS:
//   stage A   acc = W_k3 . ELU(x)      tap6_mainloop<1,4,4,1> with FUSE = 1: the raw rows are activated while they are staged (the same
//             elu1 the producers' epilogues apply, so the staged planes carry the bits the ELU'd flavour had); K = 768, N = 128
//   hand-over hidden = ELU(2^-s acc + b3), split with the scale of the derived bound |hidden| <= hb0 + hb1 amax(x) (rb_params6.h,
//             as the other fused blocks: the two-launch path scales by the hidden tensor's MEASURED amax, which a fused kernel cannot
//             know before its tile is done -- the only arithmetic difference between the two paths), written over the dead A slab
//   stage B   acc = W_1x1 . hidden  (8 k-steps, operand fragments from the hidden planes)  +  W_sc . x  (tap6_mainloop<1,4,4,2> with
//             FUSE = 2 over the raw rows, k offset 128): the k order of the two-launch path's [hidden | x] contraction
//   epilogue  tap6_epilogue of the 128 x 256 tile: bias, ELU'd (and optionally raw) output, the clip's amax.
// LDS: max(hidden planes 68 KB, A slab 42 KB, epilogue staging) -- two workgroups per CU.  The regions overlay each other, every
// hand-over is fenced by a workgroup barrier.  No counted wait of its own: the waits are tap6_mainloop's.
#pragma once
#include "tap_gemm6.h"
#include "rb_params6.h"

namespace ac {

struct Rb256Params {
    TapGemmParams a;        // stage A: one segment (the raw rows, 3 taps), N = 128, Ktot = 768; bias, winv; no outputs
    TapGemmParams b;        // stage B: one segment (the raw rows, 1 tap, kofs = 128), N = 256, Ktot = 384; bias, winv, outputs, amax_out
    float hb0, hb1;         // |hidden| <= hb0 + hb1 amax(x)
};

struct Rb256Cfg {
    using CA = Tap6Cfg<1, 4, 4, 1, 7>;
    using CB = Tap6Cfg<1, 4, 4, 2, 7>;
    static constexpr int BM = 128, HC = 128, NT = 256;
    static constexpr int HP = HC + 8;                       // fp16 per hidden row: 272-byte rows keep 16-byte alignment, spread banks
    static constexpr int H_PLANE = BM * HP;
    static constexpr size_t h_bytes = (size_t)2 * H_PLANE * 2;
    static constexpr size_t ab_bytes = CA::lds_bytes > CB::lds_bytes ? CA::lds_bytes : CB::lds_bytes;
    static constexpr size_t lds_bytes = h_bytes > ab_bytes ? h_bytes : ab_bytes;
    static_assert(CA::BM == BM && CB::BM == BM && CA::BN == HC && CB::BN == 256 && 2 * lds_bytes <= 160 * 1024, "one tile shape; two workgroups per CU");
};

__global__ __launch_bounds__(256, 2) void rb256_fused_kernel(const Rb256Params q, const __bf16* __restrict__ wa, const __bf16* __restrict__ wb) {
    using Cfg = Rb256Cfg;
    constexpr int HP = Cfg::HP, H_PLANE = Cfg::H_PLANE;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i32 = lane & 31, kh = lane >> 5;
    _Float16* Hs = reinterpret_cast<_Float16*>(smem);      // [2 planes][BM][HP]
    Tap6Tile tl;
    f32x16 acc[4][2];
    {
        // ---- stage A
        f32x16 acc_a[4][1];
        tap6_mainloop<1, 4, 4, 1, 7, false, 1>(q.a, wa, smem, acc_a, tl);
        const Rb16Scale cs = rb16_scale(*amax_at(q.a.seg[0].amax, tl.b), q.hb0, q.hb1);      // (sx is the scale stage A staged with)
        const int ng = wn * 32 + i32;
        const float bv = q.a.bias[ng];
        const float iv = tl.a_inv * q.a.winv[ng];           // exact: powers of two
        lds_barrier();                                       // every wave is done reading the A slab
        // accumulator value r of a 32 x 32 tile: row 8 (r / 4) + 4 kh + r % 4, column lane & 31
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = a * 32 + 8 * (r / 4) + 4 * kh + (r % 4);
                const float v = elu1(__fmaf_rn(acc_a[a][0][r], iv, bv));
                const _Float16 hi = (_Float16)(v * cs.sb);
                const _Float16 lo = (_Float16)__builtin_fmaf(v, cs.sb, -(float)hi);
                Hs[row * HP + ng] = hi;
                Hs[H_PLANE + row * HP + ng] = lo;
            }
        tl.a_scale = cs.sb;                                  // hidden and raw rows share stage B's accumulators, so they share a scale
        tl.a_inv = cs.ib;
    }
    lds_barrier();

    // ---- stage B, hidden part: k-steps 0 .. 7 of the [1x1 | shortcut] image; this wave's column tiles 2 wn, 2 wn + 1
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;
    {
        const int ksteps = q.b.Ktot >> 4;
        const __bf16* wbase = wb + ((long long)(wn * 2) * ksteps) * (2 * 64 * 8) + lane * 8;
        auto load_b = [&](int s, bf16x8 (&bf)[2][2]) {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) bf[pl][c] = *reinterpret_cast<const bf16x8*>(wbase + (((long long)c * ksteps + s) * 2 + pl) * (64 * 8));
        };
        const _Float16* Ha = Hs + i32 * HP + 8 * kh;
        auto step = [&](int s, const bf16x8 (&bf)[2][2]) {
            f16x8 af[2][4];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                for (int a = 0; a < 4; ++a) af[pl][a] = *reinterpret_cast<const f16x8*>(Ha + pl * H_PLANE + a * 32 * HP + s * 16);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c) {             // lo hi, hi lo, hi hi (tap6_mainloop's order)
                    f32x16 v = acc[a][c];
                    v = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[1][a], __builtin_bit_cast(f16x8, bf[0][c]), v, 0, 0, 0);
                    v = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0][a], __builtin_bit_cast(f16x8, bf[1][c]), v, 0, 0, 0);
                    acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0][a], __builtin_bit_cast(f16x8, bf[0][c]), v, 0, 0, 0);
                }
        };
        bf16x8 b0[2][2], b1[2][2];
        load_b(0, b0);
#pragma unroll
        for (int s = 0; s < Cfg::HC / 16; s += 2) {       // each weight set is requested one k-step ahead of its use
            load_b(s + 1, b1);
            step(s, b0);
            if (s + 2 < Cfg::HC / 16) load_b(s + 2, b0);
            step(s + 1, b1);
        }
    }
    lds_barrier();                                           // every wave is done reading the hidden planes: the slab may return

    // ---- stage B, shortcut part, and the tile's epilogue
    tap6_mainloop<1, 4, 4, 2, 7, false, 2>(q.b, wb, smem, acc, tl);
    tap6_epilogue<1, 4, 4, 2, 7>(q.b, acc, smem, tl.b, tl.m0, tl.n0, tl.a_inv, false, tl.clk_t0, tl.clk_r0, false);
}

}  // namespace ac
