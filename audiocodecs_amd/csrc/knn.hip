// knn.hip: the k-NN feature matcher (knn.h) -- its kernels, the choice of the split count and the handle-free
// ac_knn_* entry points.  Every refusal is decided here on the host, before anything is launched; nothing allocates or synchronises.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "metric_host.h"
#include "knn.h"

namespace ac {

static bool knn_width_ok(int H) { return H == 32 || H == 64 || H == 128 || H == 256 || H == 512; }
static bool knn_rows_ok(long long n) { return n >= 1 && n <= KNN_MAX_ROWS; }
static long long knn_mpad(long long M) { return (M + 15) / 16 * 16; }
static int knn_ms(int H) { return H == 512 ? 1 : 2; }                 // row tiles per wave (registers: two tile sets of H = 512 leave room for one)
static int knn_kl(int topk) { return topk <= 4 ? 4 : 8; }

// Slices of the table for a call that names none: enough workgroups (one wave each) for the 1024 SIMDs, while a slice keeps at least 8
// tiles (a wave's prologue -- 16 MS rows normalised and split -- and its 16-lane merge stay small beside its walk) and the finish kernel
// at most 16 lists per row.  S = 1 from 1024 query waves on, and for tables below 16 tiles.
static int knn_auto_splits(long long Q, long long M, int H) {
    const long long waves = (Q + 16 * knn_ms(H) - 1) / (16 * knn_ms(H));
    const long long ctiles = knn_mpad(M) / 16;
    long long S = (1024 + waves - 1) / waves;
    if (S > ctiles / 8) S = ctiles / 8;
    if (S > 16) S = 16;
    return S < 1 ? 1 : (int)S;
}

template <int HV>
static void knn_match_launch(const KnnMatchParams& p, int KL, hipStream_t st) {
    constexpr int MS = HV == 32 ? 1 : 2;
    const dim3 grid((unsigned)((p.Q + 16 * MS - 1) / (16 * MS)), (unsigned)p.S);
    if (KL == 4) hipLaunchKernelGGL((knn_match_kernel<HV, MS, 4>), grid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((knn_match_kernel<HV, MS, 8>), grid, dim3(64), 0, st, p);
}

}  // namespace ac

using namespace ac;

extern "C" {

size_t ac_knn_packed_bytes(long long M, int H) {
    if (!knn_rows_ok(M) || !knn_width_ok(H)) return 0;
    return (size_t)knn_mpad(M) * H * 2 * sizeof(_Float16) + (size_t)knn_mpad(M) * sizeof(unsigned);
}

int ac_knn_pack(const float* set_dev, long long M, int H, void* packed_dev, size_t packed_bytes, void* stream) {
    if (!set_dev || !packed_dev || !aligned<16>(set_dev) || !aligned<16>(packed_dev) || !knn_rows_ok(M) || !knn_width_ok(H)) return AC_EINVAL;
    if (packed_bytes < ac_knn_packed_bytes(M, H)) return AC_ENOMEM;
    const long long Mpad = knn_mpad(M);
    _Float16* image = reinterpret_cast<_Float16*>(packed_dev);
    const KnnPackParams p{set_dev, image, reinterpret_cast<unsigned*>(image + Mpad * H * 2), (int)M, H};
    hipLaunchKernelGGL(knn_pack_kernel, dim3((unsigned)(Mpad / 16)), dim3(64), 0, (hipStream_t)stream, p);
    return launch_status();
}

int ac_knn_num_splits(long long Q, long long M, int H, int num_splits) {
    if (!knn_rows_ok(Q) || !knn_rows_ok(M) || !knn_width_ok(H) || num_splits < 0 || num_splits > KNN_MAX_SPLITS) return AC_EINVAL;
    return num_splits ? num_splits : knn_auto_splits(Q, M, H);
}

size_t ac_knn_workspace_bytes(long long Q, long long M, int H, int topk, int num_splits) {
    const int S = ac_knn_num_splits(Q, M, H, num_splits);
    if (S < 1 || topk < 1 || topk > KNN_MAX_TOPK) return 0;
    return (size_t)Q * S * knn_kl(topk) * (sizeof(float) + sizeof(int));
}

int ac_knn_match(const float* query_dev, long long Q, const float* set_dev, const void* packed_dev, long long M, int H, int topk, int num_splits,
                 float* out_dev, int64_t* idx_dev, float* sim_dev, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!query_dev || !set_dev || !packed_dev || !workspace_dev || !aligned<16>(query_dev) || !aligned<16>(set_dev) || !aligned<16>(packed_dev) ||
        !aligned<16>(workspace_dev) || !aligned<16>(out_dev))
        return AC_EINVAL;
    if (topk < 1 || topk > KNN_MAX_TOPK) return AC_EINVAL;
    const int S = ac_knn_num_splits(Q, M, H, num_splits);
    if (S < 1) return AC_EINVAL;
    if (workspace_bytes < ac_knn_workspace_bytes(Q, M, H, topk, S)) return AC_ENOMEM;
    const int KL = knn_kl(topk);
    const long long Mpad = knn_mpad(M);
    const _Float16* image = reinterpret_cast<const _Float16*>(packed_dev);
    float* ws_sim = reinterpret_cast<float*>(workspace_dev);
    int* ws_idx = reinterpret_cast<int*>(ws_sim + (size_t)Q * S * KL);
    const KnnMatchParams p{query_dev, image, reinterpret_cast<const unsigned*>(image + Mpad * H * 2), ws_sim, ws_idx, (int)Q, (int)(Mpad / 16), S};
    hipStream_t st = (hipStream_t)stream;
    switch (H) {
        case 32: knn_match_launch<2>(p, KL, st); break;
        case 64: knn_match_launch<4>(p, KL, st); break;
        case 128: knn_match_launch<8>(p, KL, st); break;
        case 256: knn_match_launch<16>(p, KL, st); break;
        default: knn_match_launch<32>(p, KL, st); break;
    }
    const KnnFinishParams f{set_dev, ws_sim, ws_idx, out_dev, reinterpret_cast<long long*>(idx_dev), sim_dev, (int)Q, H, S, topk};
    if (KL == 4) hipLaunchKernelGGL(knn_finish_kernel<4>, dim3((unsigned)Q), dim3(64), 0, st, f);
    else hipLaunchKernelGGL(knn_finish_kernel<8>, dim3((unsigned)Q), dim3(64), 0, st, f);
    return launch_status();
}

}  // extern "C"
