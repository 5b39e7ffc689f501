// tokstats.hip: the token histogram and the codebook utilisation summary (tokstats.h) -- its kernels, the choice of
// the form and the handle-free ac_tokstats_* entry points.  Every refusal is decided here on the host, before anything is launched;
// nothing allocates or synchronises.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "metric_host.h"
#include "tokstats.h"

namespace ac {

static bool ts_shape_ok(int K, int C) { return K >= 1 && K <= TS_MAX_K && C >= TS_MIN_C && C <= TS_MAX_C; }

// workgroups along x: one per 4096 elements, at most 1024 (tokstats.h: what keeps a private bin from wrapping)
static unsigned ts_blocks(long long E) {
    const long long n = (E + TS_ELEMS_PER_BLOCK - 1) / TS_ELEMS_PER_BLOCK;
    return (unsigned)(n < 1 ? 1 : n > TS_MAX_BLOCKS ? TS_MAX_BLOCKS : n);
}

}  // namespace ac

using namespace ac;

extern "C" {

size_t ac_tokstats_state_bytes(int K, int C) {
    if (!ts_shape_ok(K, C)) return 0;
    return ((size_t)K * (size_t)C + 2) * sizeof(int64_t);
}

int ac_tokstats_form(int K, int C) {
    if (!ts_shape_ok(K, C)) return AC_EINVAL;
    return ts_group(K, C);
}

int ac_tokstats_accumulate(const int64_t* toks_dev, long long B, long long N, int K, int C, const int32_t* nvalid_dev, void* state_dev,
                           size_t state_bytes, void* stream) {
    if (!ts_shape_ok(K, C) || B < 0 || N < 0 || !state_dev || !aligned<8>(state_dev)) return AC_EINVAL;
    if (state_bytes < ac_tokstats_state_bytes(K, C)) return AC_ENOMEM;
    if (B == 0 || N == 0) return AC_OK;
    if (!toks_dev || !aligned<8>(toks_dev) || !aligned<4>(nvalid_dev)) return AC_EINVAL;
    if (B > TS_MAX_ELEMS / N || B * N > TS_MAX_ELEMS / K) return AC_EINVAL;
    const long long E = B * N * K;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(state_dev);
    const int G = ts_group(K, C);
    const TokstatsParams p{reinterpret_cast<const long long*>(toks_dev), nvalid_dev, counts, counts + (size_t)K * C, counts + (size_t)K * C + 1, E, N, K, C, G};
    hipStream_t st = (hipStream_t)stream;
    const bool small = E <= (1ll << 31);
    if (G > 0) {
        const dim3 grid(ts_blocks(E), (unsigned)((K + G - 1) / G));
        const size_t lds = (size_t)G * C * sizeof(unsigned);
        if (small) hipLaunchKernelGGL(tokstats_tiled_kernel<unsigned>, grid, dim3(TS_BLOCK), lds, st, p);
        else hipLaunchKernelGGL(tokstats_tiled_kernel<unsigned long long>, grid, dim3(TS_BLOCK), lds, st, p);
    } else {
        const dim3 grid(ts_blocks(E));
        if (small) hipLaunchKernelGGL(tokstats_direct_kernel<unsigned>, grid, dim3(TS_BLOCK), 0, st, p);
        else hipLaunchKernelGGL(tokstats_direct_kernel<unsigned long long>, grid, dim3(TS_BLOCK), 0, st, p);
    }
    return launch_status();
}

int ac_tokstats_summary(const void* state_dev, int K, int C, double* out_dev, void* stream) {
    if (!ts_shape_ok(K, C) || !state_dev || !out_dev || !aligned<8>(state_dev) || !aligned<8>(out_dev)) return AC_EINVAL;
    const unsigned long long* counts = reinterpret_cast<const unsigned long long*>(state_dev);
    hipLaunchKernelGGL(tokstats_summary_kernel, dim3((unsigned)K), dim3(TS_BLOCK), 0, (hipStream_t)stream, counts, counts + (size_t)K * C, C, out_dev);
    return launch_status();
}

}  // extern "C"
