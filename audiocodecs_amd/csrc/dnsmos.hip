// dnsmos.hip: the fused DNSMOS P.808 score (dnsmos.h) -- the fp64 source of the front end's tables (host), the
// launches and the handle-free ac_dnsmos_* entry points.  Every refusal is decided here on the host, before anything is launched;
// nothing allocates or synchronises.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "metric_host.h"
#include "dnsmos.h"

namespace ac {

// librosa.filters.mel(sr = 16000, n_fft = 321, n_mels = 120, fmin = 0, fmax = 8000, htk = False, norm = "slaney"), restated (DESIGN.md 8l:
// unpinned against librosa; pinned against transformers' mel_filter_bank by the tests): Slaney's scale is linear below 1 kHz (200 / 3 Hz
// per mel) and logarithmic above (27 mels per factor 6.4); the FFT frequencies are k 16000 / 321, not a linspace to 8000.
static double dm_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}
static double dm_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}
static void dm_filterbank(double* fb) {
    const double m_max = dm_hz_to_mel(8000.0);
    double f_pts[DM_MELS + 2], f_bin[DM_BINS];
    for (int i = 0; i < DM_MELS + 2; ++i) f_pts[i] = dm_mel_to_hz(m_max * i / (DM_MELS + 1));
    for (int k = 0; k < DM_BINS; ++k) f_bin[k] = k * 16000.0 / DM_NFFT;
    triangle_filterbank(fb, f_pts, DM_MELS, f_bin, DM_BINS, true);
}

struct DmShape {
    int H[4], W[4];          // the input and the three pooled sizes
    long long chunk;         // windows per pass over the workspace
};
static bool dm_shape(long long S, int H, int W, DmShape& g) {
    if (S < 1 || S > (1 << 20) || H < 8 || W < 8 || H > 4096 || W > 4096 || (long long)H * W > (1 << 22)) return false;
    g.H[0] = H;
    g.W[0] = W;
    for (int i = 1; i < 4; ++i) {
        g.H[i] = g.H[i - 1] / 2;
        g.W[i] = g.W[i - 1] / 2;
    }
    const long long c = 32ll * DM_FRAMES * DM_MELS / ((long long)H * W);      // about 190 MB of layers at the real size, and no more at any other
    g.chunk = c < 1 ? 1 : (c > 1024 ? 1024 : c);
    if (g.chunk > S) g.chunk = S;
    return true;
}
// workspace, every piece 256-byte aligned: [slots: smax C, gmax C x 64][scores S][melpow C H W][a1][a2][a3][a4]
struct DmLayout {
    size_t slots, scores, melpow, a[4], total;
};
static DmLayout dm_layout(long long S, const DmShape& g) {
    DmLayout l;
    const size_t C = (size_t)g.chunk;
    WorkspaceCursor<256> ws;
    l.slots = ws.take(C * 65 * 4);
    l.scores = ws.take((size_t)S * 4);
    l.melpow = ws.take(C * g.H[0] * g.W[0] * 4);
    const int li[4] = {1, 2, 2, 3};
    for (int i = 0; i < 4; ++i) l.a[i] = ws.take(C * g.H[li[i]] * g.W[li[i]] * 32 * 4);
    l.total = ws.at;
    return l;
}

struct DmNetArgs {
    const float* feats;      // [S][H][W] or null (then melpow mode: the front end has filled the chunk's melpow and smax)
    float* feats_out;        // [S][H][W] or null
    float* layers[4];        // caller's [S][..] or null
    float* vec_out;          // [S][64] or null
    float* score;            // [S]
};

template <bool POOL, bool GMAX>
static void dm_launch_conv(const float* in, const unsigned char* pk, int half0, int halves, float* out, unsigned* gmax, int H, int W, int CO, long long C, hipStream_t st) {
    const int tilesX = (W + DM_TX - 1) / DM_TX, tilesY = (H + DM_TY - 1) / DM_TY;
    const long long ntiles = C * tilesX * tilesY;
    const DmConvParams p{in, reinterpret_cast<const _Float16*>(pk + DM_PK_FRAG) + (long long)half0 * DM_HALF_HALVES, reinterpret_cast<const float*>(pk + DM_PK_WINV) + half0 * 32,
                         reinterpret_cast<const float*>(pk + DM_PK_BIAS) + half0 * 32, out, gmax, H, W, CO, tilesX, tilesY, (int)ntiles};
    const unsigned grid = (unsigned)(ntiles < 512 ? ntiles : 512);      // two workgroups a CU; each loads its weight image once and walks tiles
    hipLaunchKernelGGL((dm_conv_kernel<POOL, GMAX>), dim3(grid, (unsigned)halves), dim3(256), 0, st, p);
}

static void dm_clear(unsigned char* slots, const DmShape& g, hipStream_t st) {
    const int n = (int)g.chunk * 65;
    hipLaunchKernelGGL(dm_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, reinterpret_cast<unsigned*>(slots), n);
}

// the net over windows [c0, c0 + C) of the call
static void dm_net_chunk(const DmNetArgs& a, const DmShape& g, const DmLayout& l, unsigned char* ws, const unsigned char* pk, long long c0, long long C, hipStream_t st) {
    unsigned* smax = reinterpret_cast<unsigned*>(ws + l.slots);
    unsigned* gmax = smax + g.chunk;
    float* act[4];
    const int li[4] = {1, 2, 2, 3};
    for (int i = 0; i < 4; ++i)
        act[i] = a.layers[i] ? a.layers[i] + c0 * g.H[li[i]] * g.W[li[i]] * 32 : reinterpret_cast<float*>(ws + l.a[i]);
    const long long hw = (long long)g.H[0] * g.W[0];
    const DmConv1Params c1{a.feats ? a.feats + c0 * hw : nullptr, reinterpret_cast<const float*>(ws + l.melpow), smax, reinterpret_cast<const float*>(pk + DM_PK_C5), act[0],
                           a.feats_out ? a.feats_out + c0 * hw : nullptr, g.H[0], g.W[0], (int)C};
    const long long n1 = C * g.H[1] * g.W[1];
    hipLaunchKernelGGL(dm_conv1_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, c1);
    dm_launch_conv<true, false>(act[0], pk, 0, 1, act[1], nullptr, g.H[1], g.W[1], 32, C, st);
    dm_launch_conv<false, false>(act[1], pk, 1, 1, act[2], nullptr, g.H[2], g.W[2], 32, C, st);
    dm_launch_conv<true, false>(act[2], pk, 2, 1, act[3], nullptr, g.H[2], g.W[2], 32, C, st);
    dm_launch_conv<false, true>(act[3], pk, 3, 2, nullptr, gmax, g.H[3], g.W[3], 64, C, st);
    const DmTailParams t{gmax, a.feats ? nullptr : smax, reinterpret_cast<const float*>(pk + DM_PK_DENSE), a.score + c0, a.vec_out ? a.vec_out + c0 * 64 : nullptr};
    hipLaunchKernelGGL(dm_tail_kernel, dim3((unsigned)C), dim3(64), 0, st, t);
}

}  // namespace ac

using namespace ac;

extern "C" {

size_t ac_dnsmos_source_count(void) { return DM_SRC_COUNT; }

int ac_dnsmos_source(double* src_host, size_t count) {
    if (!src_host) return AC_EINVAL;
    if (count < (size_t)DM_SRC_COUNT) return AC_ENOMEM;
    for (int j = 0; j < DM_NFFT; ++j) {
        src_host[j] = cos(2.0 * M_PI * j / DM_NFFT);
        src_host[DM_NFFT + j] = sin(2.0 * M_PI * j / DM_NFFT);
    }
    dm_filterbank(src_host + 2 * DM_NFFT);
    return AC_OK;
}

size_t ac_dnsmos_tables_bytes(void) { return (size_t)DM_BASIS_HALVES * 2 + (size_t)DM_BINS * DM_MELS * 4 + 2 * DM_MELS * 4; }

int ac_dnsmos_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream) {
    if (!src_dev || !tables_dev || !aligned<16>(src_dev) || !aligned<16>(tables_dev)) return AC_EINVAL;
    if (tables_bytes < ac_dnsmos_tables_bytes()) return AC_ENOMEM;
    _Float16* basis = reinterpret_cast<_Float16*>(tables_dev);
    float* fb = reinterpret_cast<float*>(basis + DM_BASIS_HALVES);
    const DmTablesParams p{src_dev, basis, fb, reinterpret_cast<int*>(fb + DM_BINS * DM_MELS)};
    const long long threads = (long long)DM_PASSES * DM_KS * 4 * 64 + (long long)DM_BINS * DM_MELS + DM_MELS;
    hipLaunchKernelGGL(dm_tables_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status();
}

size_t ac_dnsmos_weights_count(void) { return DM_W_COUNT; }
size_t ac_dnsmos_packed_bytes(void) { return DM_PK_BYTES; }

int ac_dnsmos_pack(const float* weights_dev, size_t count, void* packed_dev, size_t packed_bytes, void* stream) {
    if (!weights_dev || !packed_dev || !aligned<4>(weights_dev) || !aligned<16>(packed_dev) || count != (size_t)DM_W_COUNT) return AC_EINVAL;
    if (packed_bytes < DM_PK_BYTES) return AC_ENOMEM;
    const DmPackParams p{weights_dev, reinterpret_cast<unsigned char*>(packed_dev)};
    const int threads = 5 * 9 * 2 * 64 + 320 + 4160 + 4160 + 65;
    hipLaunchKernelGGL(dm_pack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    return launch_status();
}

size_t ac_dnsmos_workspace_bytes(long long S, int H, int W) {
    DmShape g;
    if (!dm_shape(S, H, W, g)) return 0;
    return dm_layout(S, g).total;
}

int ac_dnsmos_net(const float* feats_dev, long long S, int H, int W, const void* packed_dev, float* score_out, float* layer1_out, float* layer2_out, float* layer3_out,
                  float* layer4_out, float* vec_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!feats_dev || !packed_dev || !score_out || !workspace_dev) return AC_EINVAL;
    if (!aligned<4>(feats_dev) || !aligned<16>(packed_dev) || !aligned<4>(score_out) || !aligned<16>(layer1_out) || !aligned<16>(layer2_out) ||
        !aligned<16>(layer3_out) || !aligned<16>(layer4_out) || !aligned<4>(vec_out) || !aligned<16>(workspace_dev))
        return AC_EINVAL;
    DmShape g;
    if (!dm_shape(S, H, W, g)) return AC_EINVAL;
    const DmLayout l = dm_layout(S, g);
    if (workspace_bytes < l.total) return AC_ENOMEM;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace_dev);
    const DmNetArgs a{feats_dev, nullptr, {layer1_out, layer2_out, layer3_out, layer4_out}, vec_out, score_out};
    for (long long c0 = 0; c0 < S; c0 += g.chunk) {
        const long long C = S - c0 < g.chunk ? S - c0 : g.chunk;
        dm_clear(ws + l.slots, g, st);
        dm_net_chunk(a, g, l, ws, reinterpret_cast<const unsigned char*>(packed_dev), c0, C, st);
    }
    return launch_status();
}

int ac_dnsmos(const float* sig_dev, long long B, long long L16, const int32_t* plan_dev, long long S, int Smax, const void* tables_dev, const void* packed_dev,
              float* score_out, float* segments_out, float* feats_out, void* workspace_dev, size_t workspace_bytes, void* stream) {
    if (!sig_dev || !plan_dev || !tables_dev || !packed_dev || !score_out || !workspace_dev) return AC_EINVAL;
    if (!aligned<4>(sig_dev) || !aligned<16>(plan_dev) || !aligned<16>(tables_dev) || !aligned<16>(packed_dev) || !aligned<4>(score_out) ||
        !aligned<4>(segments_out) || !aligned<4>(feats_out) || !aligned<16>(workspace_dev))
        return AC_EINVAL;
    DmShape g;
    if (B < 1 || B > S || L16 < 1 || L16 > DM_MAX_L || Smax < 1 || Smax > S || !dm_shape(S, DM_FRAMES, DM_MELS, g)) return AC_EINVAL;
    const DmLayout l = dm_layout(S, g);
    if (workspace_bytes < l.total) return AC_ENOMEM;
    hipStream_t st = (hipStream_t)stream;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace_dev);
    const _Float16* basis = reinterpret_cast<const _Float16*>(tables_dev);
    const float* fb = reinterpret_cast<const float*>(basis + DM_BASIS_HALVES);
    float* seg = reinterpret_cast<float*>(ws + l.scores);
    const DmNetArgs a{nullptr, feats_out, {nullptr, nullptr, nullptr, nullptr}, nullptr, seg};
    for (long long c0 = 0; c0 < S; c0 += g.chunk) {
        const long long C = S - c0 < g.chunk ? S - c0 : g.chunk;
        dm_clear(ws + l.slots, g, st);
        const DmFrontParams f{sig_dev, plan_dev + 4 * c0, basis, fb, reinterpret_cast<const int*>(fb + DM_BINS * DM_MELS), reinterpret_cast<float*>(ws + l.melpow),
                              reinterpret_cast<unsigned*>(ws + l.slots), L16, (int)B};
        hipLaunchKernelGGL(dm_front_kernel, dim3(DM_TILES, (unsigned)C), dim3(64), 0, st, f);
        dm_net_chunk(a, g, l, ws, reinterpret_cast<const unsigned char*>(packed_dev), c0, C, st);
    }
    const DmMeanParams m{seg, plan_dev + 4 * S, score_out, segments_out, (int)B, Smax, (int)S};
    hipLaunchKernelGGL(dm_mean_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, m);
    return launch_status();
}

}  // extern "C"
