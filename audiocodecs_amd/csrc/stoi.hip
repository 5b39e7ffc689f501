// stoi.hip: the fused STOI (stoi.h) -- the fp64 source of the tables (host), the launches and the handle-free
// ac_stoi_* entry points.  Every refusal is decided here on the host, before anything is launched; nothing allocates or synchronises,
// and nothing the device computes (K, the kept frames) is read back: the whole call can be captured into a graph.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "metric_host.h"
#include "stoi.h"

namespace ac {

static long long st_len10(long long L16) { return (ST_UP * L16 + ST_DOWN - 1) / ST_DOWN; }
static long long st_frames(long long L16) { return (st_len10(L16) - ST_WIN) / ST_HOP + 1; }
static bool st_shape_ok(int P, long long B, long long L16) {
    return P >= 1 && P <= ST_MAX_P && B >= 1 && L16 >= 1 && L16 <= ST_MAX_L16 && st_len10(L16) >= ST_WIN && (long long)(1 + P) * B <= 0x7fffffffll &&
           B * ((st_frames(L16) + 14) / 16 + 1) <= 0x7fffffffll / ST_MAX_P;      // (grids: one workgroup per clip and frame tile / hypothesis, clip and 16 segments)
}

// the workspace, every piece 16-byte aligned
struct StLayout {
    size_t x10, energy, src, kept, K, bad, env, segsum, total;
    long long L10, F0, NS0;
};
static StLayout st_layout(int P, long long B, long long L16) {
    StLayout l;
    l.L10 = st_len10(L16);
    l.F0 = st_frames(L16);
    l.NS0 = l.F0 > ST_SEG ? l.F0 - ST_SEG : 0;
    WorkspaceCursor<16> ws;
    l.x10 = ws.take((size_t)(1 + P) * B * l.L10 * sizeof(float));
    l.energy = ws.take((size_t)B * l.F0 * sizeof(float));
    l.src = ws.take((size_t)B * l.F0 * sizeof(int));
    l.kept = ws.take((size_t)B * l.F0);
    l.K = ws.take((size_t)B * sizeof(int));
    l.bad = ws.take((size_t)(1 + P) * B * sizeof(int));
    l.env = ws.take((size_t)(1 + P) * B * l.F0 * 16 * sizeof(float));
    l.segsum = ws.take((size_t)P * B * l.NS0 * sizeof(float));
    l.total = ws.at;
    return l;
}

// modified Bessel function of the first kind, order 0: the power series (x <= 6 here: 40 terms leave nothing)
static double st_i0(double x) {
    double term = 1.0, sum = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 40; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}

// pystoi's resample_oct(x, 10000, 16000) filter (restated: DESIGN.md 8k, unpinned): Kaiser-windowed sinc, 60 dB, roll-off fc / 10, normalised
// to sum 1 and multiplied by `up`
static void st_fir(double* h) {
    const double fc = 1.0 / (2.0 * ST_DOWN), beta = 0.1102 * (60.0 - 8.7);
    const int L = ST_FIR_HALF;
    double sum = 0.0;
    for (int t = -L; t <= L; ++t) {
        const double r = (double)t / L;
        const double win = st_i0(beta * sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / st_i0(beta);
        const double a = M_PI * 2.0 * fc * t;
        const double sinc = t == 0 ? 1.0 : sin(a) / a;
        h[t + L] = win * 2.0 * ST_UP * fc * sinc;
        sum += h[t + L];
    }
    for (int i = 0; i <= 2 * L; ++i) h[i] = ST_UP * h[i] / sum;
}

}  // namespace ac

using namespace ac;

extern "C" {

size_t ac_stoi_source_count(void) { return ST_SRC_COUNT; }

int ac_stoi_source(double* src_host, size_t count) {
    if (!src_host) return AC_EINVAL;
    if (count < (size_t)ST_SRC_COUNT) return AC_ENOMEM;
    for (int n = 0; n < ST_WIN; ++n) src_host[n] = 0.5 * (1.0 - cos(2.0 * M_PI * (n + 1) / (ST_WIN + 1)));      // hanning(258)[1:-1]
    for (int j = 0; j < ST_NFFT; ++j) src_host[ST_WIN + j] = cos_turn(j, ST_NFFT);
    st_fir(src_host + ST_WIN + ST_NFFT);
    return AC_OK;
}

size_t ac_stoi_tables_bytes(void) { return ST_WINDOW_BYTES + ST_FIR_BYTES + (size_t)ST_BASIS_HALVES * sizeof(_Float16); }

int ac_stoi_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream) {
    if (!src_dev || !tables_dev || !aligned<16>(src_dev) || !aligned<16>(tables_dev)) return AC_EINVAL;
    if (tables_bytes < ac_stoi_tables_bytes()) return AC_ENOMEM;
    char* t = reinterpret_cast<char*>(tables_dev);
    const StTablesParams p{src_dev, reinterpret_cast<float*>(t), reinterpret_cast<float*>(t + ST_WINDOW_BYTES), reinterpret_cast<_Float16*>(t + ST_WINDOW_BYTES + ST_FIR_BYTES)};
    const int threads = ST_TILES * ST_KS * 2 * 64 + ST_WIN + ST_UP * ST_FIR_TAPS;
    hipLaunchKernelGGL(stoi_tables_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status();
}

long long ac_stoi_num_frames(long long L16) { return L16 >= 1 && L16 <= ST_MAX_L16 && st_len10(L16) >= ST_WIN ? st_frames(L16) : 0; }

size_t ac_stoi_workspace_bytes(int P, long long B, long long L16) { return st_shape_ok(P, B, L16) ? st_layout(P, B, L16).total : 0; }

int ac_stoi(const float* hyp_dev, const float* ref_dev, int P, long long B, long long L16, const void* tables_dev, float* score_out, uint8_t* kept_out,
            int32_t* num_segments_out, float* segments_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!hyp_dev || !ref_dev || !tables_dev || !score_out || !workspace_dev) return AC_EINVAL;
    if (!aligned<4>(hyp_dev) || !aligned<4>(ref_dev) || !aligned<16>(tables_dev) || !aligned<16>(workspace_dev) || !aligned<4>(score_out) ||
        !aligned<4>(num_segments_out) || !aligned<4>(segments_out))
        return AC_EINVAL;
    if (!st_shape_ok(P, B, L16)) return AC_EINVAL;
    const StLayout l = st_layout(P, B, L16);
    if (workspace_bytes < l.total) return AC_ENOMEM;
    hipStream_t st = (hipStream_t)stream;
    const char* t = reinterpret_cast<const char*>(tables_dev);
    const float* window = reinterpret_cast<const float*>(t);
    const float* fir = reinterpret_cast<const float*>(t + ST_WINDOW_BYTES);
    const _Float16* basis = reinterpret_cast<const _Float16*>(t + ST_WINDOW_BYTES + ST_FIR_BYTES);
    char* ws = reinterpret_cast<char*>(workspace_dev);
    float* x10 = reinterpret_cast<float*>(ws + l.x10);
    int* K = reinterpret_cast<int*>(ws + l.K);
    int* bad = reinterpret_cast<int*>(ws + l.bad);
    int* src = reinterpret_cast<int*>(ws + l.src);
    float* env = reinterpret_cast<float*>(ws + l.env);
    float* segsum = reinterpret_cast<float*>(ws + l.segsum);
    const int iB = (int)B, L10 = (int)l.L10, F0 = (int)l.F0, NS0 = (int)l.NS0;

    // 16 kHz -> 10 kHz: the reference's rows, then the hypotheses' (one fp32 fma chain per output, ascending taps)
    int rc = ac_resample(ref_dev, iB, (int)L16, fir, ST_UP, ST_DOWN, ST_FIR_TAPS, ST_FIR_WIDTH, x10, L10, stream);
    if (rc != AC_OK) return rc;
    rc = ac_resample(hyp_dev, P * iB, (int)L16, fir, ST_UP, ST_DOWN, ST_FIR_TAPS, ST_FIR_WIDTH, x10 + (size_t)B * l.L10, L10, stream);
    if (rc != AC_OK) return rc;

    const StMaskParams m{x10, window, reinterpret_cast<float*>(ws + l.energy), src, K, bad, reinterpret_cast<uint8_t*>(ws + l.kept), kept_out, num_segments_out, iB, L10, F0};
    hipLaunchKernelGGL(stoi_mask_kernel, dim3((unsigned)B, (unsigned)(1 + P)), dim3(256), 0, st, m);
    const int tiles = (F0 - 1 + ST_FT - 1) / ST_FT;      // STFT frames of the rebuilt signal: K - 1 <= F0 - 1
    if (tiles > 0) {
        const StBandsParams bp{x10, window, basis, src, K, env, iB, L10, F0, tiles, 1 + P};
        hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)(B * tiles)), dim3(256), 0, st, bp);
    }
    if (NS0 > 0) {
        const int chunks = (NS0 + 15) / 16;
        const StSegParams sp{env, K, segsum, iB, F0, NS0, chunks};
        hipLaunchKernelGGL(stoi_segments_kernel, dim3((unsigned)((long long)P * B * chunks)), dim3(256), 0, st, sp);
    }
    const StFinishParams fp{segsum, K, bad, score_out, segments_out, iB, NS0};
    hipLaunchKernelGGL(stoi_finish_kernel, dim3((unsigned)(P * B)), dim3(64), 0, st, fp);
    return launch_status();
}

}  // extern "C"
