// tap_route.h: which tap-GEMM kernel run_tap (core.hip) launches for a layer, as a pure function of the layer's parameters, what
// the packer made of its weights and the developer switches.  No HIP call, no handle state, no environment: ac_debug_tap_route
// (ac_api.hip) runs it on the CPU, tests/test_tap_route.py holds the choices for the four codecs' layers.
#pragma once
#include "core.h"

namespace acimpl {

// what route_tap cannot see in TapGemmParams
struct TapRouteInputs {
    bool w6 = false;             // the weights have split16 bf16 planes (ac_handle::w6_of)
    bool winv = false;           // ... and per-row 2^-s (ac_handle::winv_of)
    bool want_rowmode = false;   // the caller asked for row mode (TapGemmParams::amax_rows on entry)
    bool want_rows = false;      // ... and for the output's row words (amax_out_rows on entry)
    bool gemm_fp32 = false;      // exact-fp32 products only
};

enum class TapFamily { scalar, vec, tap4, tap6, tap6_dil, tap8 };

// the template arguments of a launch as one switch key (tap_gemm*_kernel<WGM, WGN, WM|WMT, WN, ...> and tap_gemm8's flags)
enum { TK_RM = 1, TK_J1 = 2, TK_SPREAD = 4 };
constexpr int tap_key(int wgm, int wgn, int wm, int wn, int flags = 0) { return flags << 16 | wgm << 12 | wgn << 8 | wm << 4 | wn; }

struct TapRoute {
    int reject_taps = 0;          // > 0: a segment has this many taps, more than any kernel takes (run_tap fails)
    TapFamily family = TapFamily::scalar;
    int wgm = 0, wgn = 0, wm = 0, wn = 0;   // arrangement (wm: WMT of tap_gemm6 / tap_gemm8)
    int form8 = 0;                // tap_gemm8 tile form: 1 = 256 x 256, 2 = 256 x 128, 3 = 128 x 256
    bool rm = false, j1 = false, spread = false;   // tap_gemm8's RM / J1 / SPREAD
    bool rowmode = false;         // split16.h row mode: one scale per row of a merged row matrix
    bool rows_out = false;        // ... with the output's row words (TapGemmParams::amax_out_rows)
    bool epi_direct = false;      // TapGemmParams::epi_direct
    bool dil_slab = false;        // dilated taps may come out of one wide slab (family tap6_dil where the arrangement gains)
    char name[48] = "";           // profile record name, without the prof_detail shape suffix
    int key() const { return tap_key(wgm, wgn, wm, wn, (rm ? TK_RM : 0) | (j1 ? TK_J1 : 0) | (spread ? TK_SPREAD : 0)); }
};

inline void tap_route_set(TapRoute& r, TapFamily f, int wgm, int wgn, int wm, int wn) {
    r.family = f;
    r.wgm = wgm;
    r.wgn = wgn;
    r.wm = wm;
    r.wn = wn;
    const char* fmt = f == TapFamily::scalar   ? "tap_gemm_kernel<%d, %d, %d, %d, false>"
                      : f == TapFamily::vec    ? "tap_gemm_kernel<%d, %d, %d, %d, true>"
                      : f == TapFamily::tap4   ? "tap_gemm4_kernel<%d, %d, %d, %d>"
                      : f == TapFamily::tap6   ? "tap_gemm6_kernel<%d, %d, %d, %d, 2>"
                      : f == TapFamily::tap6_dil ? "tap_gemm6_kernel<%d, %d, %d, %d, 2, dil>"
                                                 : "tap_gemm8_kernel<%d, %d, %d, %d, 2>";
    std::snprintf(r.name, sizeof r.name, fmt, wgm, wgn, wm, wn);
}

inline TapRoute route_tap(const TapGemmParams& p, const TapRouteInputs& in, const ac_handle::DevSwitches& dev) {
    TapRoute r;
    bool vec = (p.Ktot % 4 == 0) && aligned16(p.w);
    bool fast = vec && (p.N % 4 == 0) && (p.y_rs % 4 == 0) && (p.y_bs % 4 == 0) && (!p.y || aligned16(p.y)) &&
                (!p.y_elu || aligned16(p.y_elu)) && (long long)p.N * p.Ktot * 4 < (1LL << 31);
    for (int i = 0; i < p.nseg; ++i) {
        const TapSeg& s = p.seg[i];
        vec = vec && (s.cin % 4 == 0) && (s.ts % 4 == 0) && (s.bs % 4 == 0) && (s.kofs % 4 == 0) && aligned16(s.x);
        fast = fast && ((s.s * s.cin) % KC == 0) && (s.ts == s.cin || s.s == 1) && !s.rel_len && !s.elu &&
               ((long long)(s.L - 1) * s.ts + s.cin) * 4 < (1LL << 31);
        if (s.J > 8) {
            r.reject_taps = s.J;
            return r;
        }
    }
    fast = fast && vec;
    double kk = 0;
    for (int i = 0; i < p.nseg; ++i) kk += (double)p.seg[i].J * p.seg[i].s * p.seg[i].cin;
    // split-operand kernels on the bf16 pipe (tap_gemm6.h, tap_gemm8.h) where the shape allows and the weights were packed for them
    bool use6 = fast && !in.gemm_fp32 && (p.N % 64 == 0 || p.N % 96 == 0) && in.w6;
    for (int i = 0; use6 && i < p.nseg; ++i) use6 = p.seg[i].kofs % 32 == 0;
    if (!use6) {
        const TapFamily f = fast ? TapFamily::tap4 : vec ? TapFamily::vec : TapFamily::scalar;
        if (p.N <= 16) tap_route_set(r, f, 4, 1, 2, 1);
        else if (p.N <= 32) tap_route_set(r, f, 4, 1, 2, 2);
        else if (p.N <= 64) tap_route_set(r, f, 2, 2, 2, 2);
        else if (p.N % 96 == 0 && p.N % 128 != 0) tap_route_set(r, f, 2, 2, 4, 3);   // DAC widths 96 / 192: 128-column tiles would idle a quarter of the MFMAs
        else tap_route_set(r, f, 2, 2, 4, 4);
        return r;
    }
    // (row mode only on the caller's request -- the linear layers over merged token matrices: a conv that merely happens to
    // run with one clip must scale like the same conv in a batch, or a clip's result would depend on the batch size)
    r.rowmode = in.want_rowmode && in.winv && p.B == 1 && p.nseg == 1 && p.seg[0].J == 1 && p.seg[0].s == 1 && p.seg[0].pad == 0 &&
                p.seg[0].lim >= p.M && p.seg[0].L >= p.M && p.y_off == 0;
    r.rows_out = r.rowmode && in.want_rows;
    if (!r.rowmode && in.winv) {
        // plain conv outputs store straight from the accumulators (tap_gemm6.h); AC_TAP_EPI=staged: the LDS-staged epilogue
        const bool staged_env = dev.tap_epi_staged != 0;       // (ac_debug_set "tap_epi_staged": a test flips it)
        // (ELU flavour without a residual, Snake flavour with or without one: the combinations the four codecs produce)
        r.epi_direct = !staged_env && !p.gelu && !p.scale && !p.tanh_out && p.y_off == 0 && p.y_len == 0 &&
                       (!p.res || (p.alpha && (long long)p.M * p.res_rs * 4 < 0x7fffffffLL && p.res_rs * 4 < (1 << 20))) && (!p.alpha || p.y_elu) &&
                       (p.n_valid == 0 || p.n_valid == p.N) && (p.alpha ? p.N < 128 && p.N % 32 == 0 : p.N % 128 == 0) &&      // (measured: Snake / residual layers of 128+ channels are faster through the LDS-staged 16-byte rows)
                       (long long)p.M * p.y_rs * 4 < 0x7fffffffLL && p.y_rs * 4 < (1 << 20);
    }
    const bool dil_env = dev.tap_dil != 0;                 // developer / tests: 0 -> slab reload per tap
    r.dil_slab = dil_env && !r.rowmode && p.nseg == 1 && p.seg[0].dil != 1   /* (the wide-slab instantiation has no row mode: CAN_ROWMODE, tap_gemm6.h) */ && p.seg[0].s == 1 && (p.seg[0].J - 1) * p.seg[0].dil <= T6_DIL_HALO;
    // tap_gemm8.h: the 256-row, 8-wave kernel with the weight stage through an LDS-DMA ring and activation chunks requested two
    // chunks ahead -- one segment, taps inside one slab, N % 128 == 0 (the same arithmetic in the same order: bit-identical outputs)
    const TapSeg& s0 = p.seg[0];
    const bool can8 = in.winv && p.nseg == 1 && (s0.J - 1) * s0.dil <= 7 && !(s0.dil != 1 && s0.s != 1) && p.N % 128 == 0 && (s0.s * s0.cin) % 32 == 0 &&
                      (!r.epi_direct || p.N % 128 == 0);
    const int want8 = dev.tap8;       // 0: never, 1: wherever the shape allows (developer A/B), -1: cost model
    if (can8 && want8 != 0) {
        // tile forms (8 waves each): 1 = 256 x 256 (2 x 4 waves of 128 x 64), 3 = 128 x 256 (2 x 4 waves of 64 x 64) where 256-row
        // tiles would leave CUs idle or rows empty (M = 750: three tiles per clip; M = 125), 2 = 256 x 128 (4 x 2 waves of 64 x 64) for
        // N % 256 != 0.  Score = rate relative to form 1 (EnCodec / Mimi / DAC layers, profiles/r4_tapgemm8.md) x how evenly the
        // workgroups fill the 256 CUs x the share of tile rows that exist.
        auto fill8 = [&](int bm, int bn) {
            const double w = (double)p.B * cdiv(p.M, bm) * (p.N / bn) / 256.0;
            return w / std::ceil(w) * ((double)p.M / ((double)cdiv(p.M, bm) * bm));
        };
        const double sc1 = p.N % 256 == 0 ? 1.00 * fill8(256, 256) : 0.0;
        const double sc3 = p.N % 256 == 0 ? 0.90 * fill8(128, 256) : 0.0;
        int form = sc1 >= sc3 ? 1 : 3;
        bool model = (form == 1 ? sc1 : sc3) >= 0.80;
        if (p.N % 256 != 0) {      // 64 x 64 wave tiles over 128 columns lose to tap_gemm6's three workgroups per CU except on long contractions
            form = 2;
            model = kk >= 3072 && fill8(256, 128) >= 0.70;
        }
        // tiny launches (the batch-1 / batch-8 regime: at most 64 tiles of 128 x 128): every workgroup has a CU of its own and walks its K
        // loop at one memory round trip per stage -- the ring's deeper look-ahead is what counts (1.39 -> 1.34 ms per 1 s call)
        if ((double)p.B * cdiv(p.M, 128) * (p.N / 128) <= 64.0) {
            form = p.N % 256 == 0 ? 3 : 2;
            model = true;
        }
        if (dev.tap8_form >= 1 && dev.tap8_form <= 3 && (dev.tap8_form == 2 || p.N % 256 == 0)) form = dev.tap8_form;
        if (want8 >= 1 || model) {
            r.form8 = form;
            if (form == 1) tap_route_set(r, TapFamily::tap8, 2, 4, 4, 2);
            else if (form == 3) tap_route_set(r, TapFamily::tap8, 2, 4, 2, 2);
            else tap_route_set(r, TapFamily::tap8, 4, 2, 2, 2);
            r.j1 = s0.J == 1;
            r.rm = r.j1 && r.rowmode;       // (row mode is a one-tap affair)
            // requests dealt between the MFMA units (tap_gemm8.h SPREAD): measured per form -- 128 x 256 tiles gain, 256 x 256 are level, 256 x 128 lose
            r.spread = dev.tap8_spread == 2 || (dev.tap8_spread == 1 && r.wgm * r.wm * 32 == 128);
            return r;
        }
    }
    // Tile / wave arrangement (measured, profiles/r2_tapgemm_variants.md).  The weight fragments come L2 -> registers and the
    // activation slab is shared through LDS, so the CU's vector-memory path and the LDS pipe are what an arrangement must
    // spare:  1 x 4 waves of 128 x 32 (distinct weight fragments per wave) beats 2 x 2 waves of 64 x 64 by 5-7 %;
    // 1 x 4 waves of 128 x 64 over 256 columns (half the A-slab reads, loads and splits per MFMA; lean main loop) gains
    // another 8-10 % where the launch still fills the chip evenly; 1 x 8 waves over 256 columns (one workgroup per CU)
    // wins for long contractions.  Choice by a small cost model: rate of the arrangement x how evenly its workgroups
    // fill the 256 CUs (waves of workgroups / ceil(waves)).
    int pick = 0;   // 0: 128 columns, 1: 256 columns lean, 2: 256 columns 1 x 8
    if (p.N % 256 == 0) {
        const double wg256 = (double)p.B * cdiv(p.M, 128) * (p.N / 256);
        auto fill = [](double wgs, double slots) { const double w = wgs / slots; return w / std::ceil(w); };
        // (split16: the 128-column arrangement runs three workgroups per CU and is 6 % faster per flop than before)
        const double s128 = in.winv ? 1.06 * fill(2.0 * wg256, 768.0) : 1.00 * fill(2.0 * wg256, 512.0);
        const double s256 = 1.10 * fill(wg256, 512.0);
        // (split16: 1 x 8 waves no longer beat the three-workgroup 128-column arrangement per flop -- WavTokenizer's K = 2304 layers:
        //  4.71 ms at 128 columns, 5.43 ms with 1 x 8 waves)
        const double s8 = (kk >= 2048 ? (in.winv ? 1.00 : 1.12) : (in.winv ? 0.85 : 0.95)) * fill(wg256, 256.0);
        pick = s256 >= s128 && s256 >= s8 ? 1 : (s8 > s128 ? 2 : 0);
        if (dev.tap_pick >= 0 && dev.tap_pick <= 2) pick = dev.tap_pick;     // developer override
    }
    // (256-row, 8-wave arrangements of THIS kernel -- <2,4,4,2>, <2,4,4,1> -- measured 7-12 % / 25-30 % slower per layer than
    //  the picks below: one workgroup per CU and the old load pipeline; profiles/r4_tapgemm8.md.  tap_gemm8.h is that tile with a
    //  pipeline built for it.)
    // dilated taps out of one wide slab (tap_gemm6.h: T6_DIL_HALO); measured per arrangement on DAC's layers: the 128 x 32
    // tile loses its third workgroup per CU to the larger slab and gains only for long contractions, 64 x 32 tiles lose
    auto tap6 = [&](int wgm, int wgn, int wmt, int wn) {
        const bool dil = in.winv && r.dil_slab && (wn >= 2 || (wgm == 1 && wgn == 4 && kk >= 2048));
        tap_route_set(r, dil ? TapFamily::tap6_dil : TapFamily::tap6, wgm, wgn, wmt, wn);
    };
    if (pick == 1) tap6(1, 4, 4, 2);
    else if (pick == 2) tap6(1, 8, 4, 1);
    else if (p.N % 128 == 0) tap6(1, 4, 4, 1);
    else if (p.N % 192 == 0) tap6(2, 2, 2, 3);   // DAC's 192-wide layers: a weight fragment is loaded by two waves, not four
    else if (p.N % 96 == 0) tap6(4, 1, 1, 3);
    else tap6(2, 2, 2, 1);
    return r;
}

}  // namespace acimpl
