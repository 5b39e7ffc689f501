// specdist.hip: the fused STFT / mel spectral distances (specdist.h) -- the fp64 source of the tables (host), the
// launches and the handle-free ac_specdist_* entry points.  Every refusal is decided here on the host, before anything is launched;
// nothing allocates or synchronises.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "audiocodecs_amd.h"
#include "specdist.h"

namespace ac {

static bool sd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool sd_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }      // (signals and results: fp32, read and written singly)
static bool sd_shape_ok(int P, long long B, long long L) { return P >= 1 && P <= SD_MAX_P && B >= 1 && B <= 0x7fffffffll && L > SD_NFFT / 2 && L <= SD_MAX_L; }
static long long sd_frames(long long L) { return 1 + L / SD_HOP; }
static long long sd_tiles(long long L) { return (sd_frames(L) + SD_FT - 1) / SD_FT; }
static size_t sd_basis_bytes() { return (size_t)SD_BASIS_HALVES * sizeof(_Float16); }

// cos(2 pi j / 1024) with the argument reduced to the first octant as an integer: exact at the multiples of a quarter turn
static double sd_cos1024(int j) {
    j &= 1023;
    const int q = j >> 8, r = j & 255;
    const double u = M_PI / 512.0;
    const double cs = r <= 128 ? cos(r * u) : sin((256 - r) * u), sn = r <= 128 ? sin(r * u) : cos((256 - r) * u);
    return q == 0 ? cs : q == 1 ? -sn : q == 2 ? -cs : sn;
}

// torchaudio's melscale_fbanks(513, 0, 8000, 80, 16000, norm=None, mel_scale="htk"), restated (unpinned)
static void sd_filterbank(double* fb) {
    const double m_max = 2595.0 * log10(1.0 + 8000.0 / 700.0);
    double f_pts[SD_MELS + 2];
    for (int i = 0; i < SD_MELS + 2; ++i) f_pts[i] = 700.0 * (pow(10.0, (m_max * i / (SD_MELS + 1)) / 2595.0) - 1.0);
    f_pts[SD_MELS + 1] = 8000.0;      // the last point maps back to f_max by definition: rows 0 and 512 are exactly zero
    for (int k = 0; k < SD_BINS; ++k) {
        const double f = 8000.0 * k / (SD_BINS - 1);
        for (int m = 0; m < SD_MELS; ++m) {
            const double down = (f - f_pts[m]) / (f_pts[m + 1] - f_pts[m]), up = (f_pts[m + 2] - f) / (f_pts[m + 2] - f_pts[m + 1]);
            const double v = down < up ? down : up;
            fb[k * SD_MELS + m] = v > 0.0 ? v : 0.0;
        }
    }
}

}  // namespace ac

using namespace ac;

extern "C" {

size_t ac_specdist_source_count(void) { return SD_SRC_COUNT; }

int ac_specdist_source(double* src_host, size_t count) {
    if (!src_host) return AC_EINVAL;
    if (count < (size_t)SD_SRC_COUNT) return AC_ENOMEM;
    for (int j = 0; j < SD_NFFT; ++j) src_host[j] = sd_cos1024(j);
    sd_filterbank(src_host + SD_NFFT);
    return AC_OK;
}

size_t ac_specdist_tables_bytes(void) { return sd_basis_bytes() + (size_t)SD_FB_HALVES * sizeof(_Float16); }

int ac_specdist_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream) {
    if (!src_dev || !tables_dev || !sd_aligned16(src_dev) || !sd_aligned16(tables_dev)) return AC_EINVAL;
    if (tables_bytes < ac_specdist_tables_bytes()) return AC_ENOMEM;
    _Float16* basis = reinterpret_cast<_Float16*>(tables_dev);
    const SdTablesParams p{src_dev, basis, basis + SD_BASIS_HALVES};
    const long long threads = (long long)SD_PASSES * SD_KS * 4 * 64 + (long long)SD_PASSES * SD_MT * 64;
    hipLaunchKernelGGL(sd_tables_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return hipGetLastError() == hipSuccess ? AC_OK : AC_EHIP;
}

long long ac_specdist_num_frames(long long L) { return L > SD_NFFT / 2 && L <= SD_MAX_L ? sd_frames(L) : 0; }

size_t ac_specdist_workspace_bytes(int P, long long B, long long L) {
    if (!sd_shape_ok(P, B, L) || P * B * sd_tiles(L) > 0x7fffffffll) return 0;      // (one workgroup per hypothesis, clip and tile)
    return (size_t)2 * P * B * sd_frames(L) * sizeof(float);
}

int ac_specdist(const float* hyp_dev, const float* ref_dev, int P, long long B, long long L, const void* tables_dev, float* stft_out, float* mel_out,
                float* stft_frames_out, float* mel_frames_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!hyp_dev || !ref_dev || !tables_dev || !stft_out || !mel_out || !workspace_dev) return AC_EINVAL;
    if (!sd_aligned4(hyp_dev) || !sd_aligned4(ref_dev) || !sd_aligned16(tables_dev) || !sd_aligned16(workspace_dev) || !sd_aligned4(stft_out) ||
        !sd_aligned4(mel_out) || !sd_aligned4(stft_frames_out) || !sd_aligned4(mel_frames_out))
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
    return hipGetLastError() == hipSuccess ? AC_OK : AC_EHIP;
}

}  // extern "C"
