// specdist.hip: the fused STFT / mel spectral distances (specdist.h) -- the fp64 source of the tables (host), the
// launches and the handle-free ac_specdist_* entry points.  Every refusal is decided here on the host, before anything is launched;
// nothing allocates or synchronises.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "metric_host.h"
#include "specdist.h"

namespace ac {

static bool sd_shape_ok(int P, long long B, long long L) { return P >= 1 && P <= SD_MAX_P && B >= 1 && B <= 0x7fffffffll && L > SD_NFFT / 2 && L <= SD_MAX_L; }
static long long sd_frames(long long L) { return 1 + L / SD_HOP; }
static long long sd_tiles(long long L) { return (sd_frames(L) + SD_FT - 1) / SD_FT; }
static size_t sd_basis_bytes() { return (size_t)SD_BASIS_HALVES * sizeof(_Float16); }

// torchaudio's melscale_fbanks(513, 0, 8000, 80, 16000, norm=None, mel_scale="htk"), restated (unpinned)
static void sd_filterbank(double* fb) {
    const double m_max = 2595.0 * log10(1.0 + 8000.0 / 700.0);
    double f_pts[SD_MELS + 2], f_bin[SD_BINS];
    for (int i = 0; i < SD_MELS + 2; ++i) f_pts[i] = 700.0 * (pow(10.0, (m_max * i / (SD_MELS + 1)) / 2595.0) - 1.0);
    f_pts[SD_MELS + 1] = 8000.0;      // the last point maps back to f_max by definition: rows 0 and 512 are exactly zero
    for (int k = 0; k < SD_BINS; ++k) f_bin[k] = 8000.0 * k / (SD_BINS - 1);
    triangle_filterbank(fb, f_pts, SD_MELS, f_bin, SD_BINS, false);
}

}  // namespace ac

using namespace ac;

extern "C" {

size_t ac_specdist_source_count(void) { return SD_SRC_COUNT; }

int ac_specdist_source(double* src_host, size_t count) {
    if (!src_host) return AC_EINVAL;
    if (count < (size_t)SD_SRC_COUNT) return AC_ENOMEM;
    for (int j = 0; j < SD_NFFT; ++j) src_host[j] = cos_turn(j, SD_NFFT);
    sd_filterbank(src_host + SD_NFFT);
    return AC_OK;
}

size_t ac_specdist_tables_bytes(void) { return sd_basis_bytes() + (size_t)SD_FB_HALVES * sizeof(_Float16); }

int ac_specdist_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream) {
    if (!src_dev || !tables_dev || !aligned<16>(src_dev) || !aligned<16>(tables_dev)) return AC_EINVAL;
    if (tables_bytes < ac_specdist_tables_bytes()) return AC_ENOMEM;
    _Float16* basis = reinterpret_cast<_Float16*>(tables_dev);
    const SdTablesParams p{src_dev, basis, basis + SD_BASIS_HALVES};
    const long long threads = (long long)SD_PASSES * SD_KS * 4 * 64 + (long long)SD_PASSES * SD_MT * 64;
    hipLaunchKernelGGL(sd_tables_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status();
}

long long ac_specdist_num_frames(long long L) { return L > SD_NFFT / 2 && L <= SD_MAX_L ? sd_frames(L) : 0; }

size_t ac_specdist_workspace_bytes(int P, long long B, long long L) {
    if (!sd_shape_ok(P, B, L) || P * B * sd_tiles(L) > 0x7fffffffll) return 0;      // (one workgroup per hypothesis, clip and tile)
    return (size_t)2 * P * B * sd_frames(L) * sizeof(float);
}

int ac_specdist(const float* hyp_dev, const float* ref_dev, int P, long long B, long long L, const void* tables_dev, float* stft_out, float* mel_out,
                float* stft_frames_out, float* mel_frames_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!hyp_dev || !ref_dev || !tables_dev || !stft_out || !mel_out || !workspace_dev) return AC_EINVAL;
    if (!aligned<4>(hyp_dev) || !aligned<4>(ref_dev) || !aligned<16>(tables_dev) || !aligned<16>(workspace_dev) || !aligned<4>(stft_out) ||
        !aligned<4>(mel_out) || !aligned<4>(stft_frames_out) || !aligned<4>(mel_frames_out))
        return AC_EINVAL;
    const size_t need = ac_specdist_workspace_bytes(P, B, L);
    if (need == 0) return AC_EINVAL;
    if (workspace_bytes < need) return AC_ENOMEM;
    const int F = (int)sd_frames(L), tiles = (int)sd_tiles(L);
    const _Float16* basis = reinterpret_cast<const _Float16*>(tables_dev);
    float* ws = reinterpret_cast<float*>(workspace_dev);
    float* ws_mel = ws + (size_t)P * B * F;
    hipStream_t st = (hipStream_t)stream;
    const SdParams p{hyp_dev, ref_dev, basis, basis + SD_BASIS_HALVES, ws, ws_mel, (int)B, (int)L, F, tiles};
    hipLaunchKernelGGL(specdist_kernel, dim3((unsigned)(B * tiles), (unsigned)P), dim3(64), 0, st, p);
    const SdFinishParams f{ws, ws_mel, stft_out, mel_out, stft_frames_out, mel_frames_out, F};
    hipLaunchKernelGGL(specdist_finish_kernel, dim3((unsigned)(P * B)), dim3(64), 0, st, f);
    return launch_status();
}

}  // extern "C"
