// sampling.hip: fused token sampling and masked token resampling (sampling.h) -- the choice of the form and the
// handle-free ac_sample_* entry points.  Every refusal is decided here on the host, before anything is launched; nothing allocates or
// synchronises.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "metric_host.h"
#include "sampling.h"

using namespace ac;

extern "C" {

int ac_sample_form(int C) {
    if (C < SP_MIN_C || C > SP_MAX_C) return AC_EINVAL;
    return sp_form(C);
}

int ac_sample_tokens(const float* logits_dev, long long row_stride, const int64_t* row_index_dev, long long R, int C, float temp, int top_k,
                     float top_p, uint64_t key, uint64_t offset, const int64_t* offset_dev, float mask_p, const int64_t* fallback_dev,
                     int64_t* out_dev, void* stream) {
    if (!logits_dev || !out_dev || !aligned<4>(logits_dev) || !aligned<8>(out_dev)) return AC_EINVAL;
    if (!aligned<8>(row_index_dev) || !aligned<8>(offset_dev) || !aligned<8>(fallback_dev)) return AC_EINVAL;
    if (R < 0 || R > SP_MAX_ROWS || C < SP_MIN_C || C > SP_MAX_C || row_stride < C) return AC_EINVAL;
    const float scale = (float)(M_LOG2E / (double)temp);
    if (!(temp > 0.0f) || !isfinite(temp) || !isfinite(scale)) return AC_EINVAL;
    if (top_k < 0 || top_k > C || !(top_p <= 1.0f)) return AC_EINVAL;
    if (top_k > 0 && top_p >= 0.0f) return AC_EINVAL;                    // one cut at a time, as the reference
    if (!(mask_p <= 1.0f) || (mask_p >= 0.0f && !fallback_dev)) return AC_EINVAL;
    if (R == 0) return AC_OK;
    const SampleParams p{logits_dev, row_stride, reinterpret_cast<const long long*>(row_index_dev), R, C, scale, top_k, top_p,
                         (unsigned long long)key, (unsigned long long)offset, reinterpret_cast<const long long*>(offset_dev), mask_p,
                         reinterpret_cast<const long long*>(fallback_dev), reinterpret_cast<long long*>(out_dev)};
    hipStream_t st = (hipStream_t)stream;
    if (sp_form(C) == 1) {
        const unsigned blocks = (unsigned)((R + SP_ROWS_PER_BLOCK - 1) / SP_ROWS_PER_BLOCK);
        hipLaunchKernelGGL(sample_wave_kernel, dim3(blocks), dim3(64 * SP_ROWS_PER_BLOCK), 0, st, p);
    } else {
        hipLaunchKernelGGL(sample_block_kernel, dim3((unsigned)R), dim3(64u * (unsigned)sp_waves(C)), 0, st, p);
    }
    return launch_status();
}

}  // extern "C"
