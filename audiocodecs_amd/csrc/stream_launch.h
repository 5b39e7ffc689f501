// Host side of stream_stage.h: the launch sequences the streaming paths share (mimi_stream.hip, encodec_stream.hip).
#pragma once
#include "core.h"
#include "stream_stage.h"

namespace acimpl {

static unsigned grid_for(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 65536); }

static Act staged_act(const float* p, int B, int rows, int C) { return Act{p, (long long)rows * C, C, rows, C}; }

// a slot list (host memory): 1 <= n <= B entries in [0, B), none twice
static int stream_slots_check(ac_handle* h, const int* slots, int n, int B, const char* who) {
    if (n < 1 || n > B) return fail(h, AC_EINVAL, "%s: n=%d slots of a state of %d", who, n, B);
    std::vector<uint8_t> seen((size_t)B, 0);
    for (int i = 0; i < n; ++i) {
        if (slots[i] < 0 || slots[i] >= B) return fail(h, AC_EINVAL, "%s: slot %d outside [0, %d)", who, slots[i], B);
        if (seen[slots[i]]) return fail(h, AC_EINVAL, "%s: slot %d listed twice", who, slots[i]);
        seen[slots[i]] = 1;
    }
    return AC_OK;
}

// a slot call's own arguments (the rest is the push's); a null handle falls through to the push's check
static int stream_slots_args(ac_handle* h, const int* slots_host, const int* slots_dev, const char* who) {
    if (h && (!slots_host || !slots_dev)) return fail(h, AC_EINVAL, "%s: the slot list is null", who);
    return AC_OK;
}

// [cache | x] -> staged (a fresh activation buffer of B * (P + L) * C floats); x's last P rows -> cache.  `cache` [B][P][C] and
// `fresh` [B] live in the stream state; `mode` (STAGE_*) is a fresh stream's history.  `slot` (device, [B]; null = identity): the push's
// row b addresses stream slot[b] of the `slot_cap` streams the state holds; x and staged stay dense.
// (`any_L`: a chunk shorter than the history is staged in two launches -- stream_stage.h mstream_stage_ro_kernel)
static int stream_stage(ac_handle* h, hipStream_t st, float* cache, const int* fresh, int P, int C, int l, const Act& x, int B, float* staged,
                        size_t cap, int mode, bool any_L, const int* slot = nullptr, int slot_cap = 0) {
    MStreamStageParams p{};
    p.P = P;
    p.C = C;
    if (x.C != p.C) return fail(h, AC_EINVAL, "stream stage %d: %d channels, cache holds %d", l, x.C, p.C);
    if (x.L < p.P && !any_L) return fail(h, AC_EINVAL, "stream stage %d: %d rows per push, fewer than the %d history rows", l, x.L, p.P);
    if ((size_t)B * (p.P + x.L) * p.C > cap) return fail(h, AC_ENOMEM, "stream stage %d exceeds its workspace buffer", l);
    p.cache = cache;
    p.x = x.p;
    p.bs = x.bs;
    p.ts = x.ts;
    p.y = staged;
    p.fresh = fresh;
    p.B = B;
    p.L = x.L;
    p.replicate = mode;
    p.slot = slot;
    p.cap = slot ? slot_cap : B;
    const long long n = (long long)B * (p.P + x.L) * p.C;
    if (x.L < p.P) {
        {
            ProfScope ps(h, st, "mstream_stage_ro_kernel", 0.0, 8.0 * n);
            hipLaunchKernelGGL(mstream_stage_ro_kernel<>, dim3(grid_for(n)), dim3(256), 0, st, p);
            HIPCHK(h, hipGetLastError());
        }
        const long long nc = (long long)B * p.P * p.C;
        ProfScope ps(h, st, "mstream_cache_tail_kernel", 0.0, 8.0 * nc);
        hipLaunchKernelGGL(mstream_cache_tail_kernel<>, dim3(grid_for(nc)), dim3(256), 0, st, p);
        HIPCHK(h, hipGetLastError());
        return AC_OK;
    }
    ProfScope ps(h, st, "mstream_stage_kernel", 0.0, 8.0 * n);
    hipLaunchKernelGGL(mstream_stage_kernel<>, dim3(grid_for(n)), dim3(256), 0, st, p);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

// a causal conv on a staged input: M outputs, output m reads staged rows [m*s, m*s + k) (no padding left)
static int mstream_conv(ac_handle* h, hipStream_t st, const PackedGemm& g, const Act& xs, int k, int s, int M, Out out, int B, Act2* y,
                        const Epi& epi = Epi{}) {
    return tap_layer(h, st, g, {make_seg(xs, s, s == 1 ? k : 2, PAD_ZERO, 0, 0, nullptr, 0, 0)}, B, M, TapDst{out, (long long)M * g.N, g.N}, epi, y);
}

}  // namespace acimpl
