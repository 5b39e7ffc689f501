// Streaming Mimi encode (include/audiocodecs_amd.h ac_mimi_stream_*; DESIGN.md "Streaming Mimi encode").
// A push of F whole frames per stream runs the batch encoder's layers on [history | chunk]: every causal conv reads its last
// k - stride input rows from the stream state (mstream_stage_kernel, then the tap-GEMM with no left padding); the transformer's
// attention reads the K / V ring of the previous sliding_window - 1 positions (mstream_attn_kernel).  The fused batch-only blocks
// (rb_stream6m with the folded stem, rb_stream128m, rb_fused6) assume zero history: a push goes through the per-conv tap-GEMMs.
// The caller owns the state and the workspace; no entry point here allocates or synchronises.
#include "core.h"
#include "mimi_stream.h"

namespace acimpl {

// byte layout of a state buffer for B streams (every section 256-B aligned)
struct MStreamLayout {
    size_t pos = 0, fresh = 0;                 // int64 [B], int32 [B]
    std::vector<size_t> conv;                  // caches in encoder order: stem, (block k3, down-sampler) per ratio, final conv, down-sampler
    std::vector<int> conv_P, conv_C;           //   rows (k - stride) and channels of each
    size_t ring = 0;                           // per transformer layer: keys [B][R][A], then values [B][R][A]
    int R = 0, A = 0;
    size_t total = 0;
};

static MStreamLayout mstream_layout(const ac_handle* h, int B) {
    const ac_mimi_config& c = h->mcfg;
    MStreamLayout L;
    size_t off = align_up(sizeof(MStreamHeader), 256);
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    L.pos = take((size_t)B * 8);
    L.fresh = take((size_t)B * 4);
    auto conv = [&](int P, int C) { L.conv.push_back(take((size_t)B * P * C * 4)); L.conv_P.push_back(P); L.conv_C.push_back(C); };
    conv(c.kernel_size - 1, 1);
    int ch = c.num_filters;
    for (int i = 0; i < c.num_ratios; ++i) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - i];
        conv(c.residual_kernel_size - 1, ch);
        conv(ratio, ch);
        ch *= 2;
    }
    conv(c.last_kernel_size - 1, ch);
    conv(c.resample_stride, c.hidden_size);
    L.R = c.sliding_window - 1;
    L.A = c.num_attention_heads * c.head_dim;
    L.ring = off;
    off += (size_t)c.num_hidden_layers * 2 * align_up((size_t)B * L.R * L.A * 4, 256);
    L.total = off;
    return L;
}

static unsigned long long mstream_fingerprint(const ac_mimi_config& c) {
    ac_mimi_config k = c;
    k.device = 0;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&k);
    unsigned long long f = 1469598103934665603ULL;
    for (size_t i = 0; i < sizeof k; ++i) f = (f ^ b[i]) * 1099511628211ULL;
    return f;
}

static unsigned grid_for(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 65536); }

// [cache | x] -> staged (a fresh activation buffer of B * (P + L) * C floats); x's last P rows -> cache
static int mstream_stage(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, int l, const Act& x, int B, float* staged,
                         size_t cap, bool replicate) {
    MStreamStageParams p{};
    p.P = Ls.conv_P[l];
    p.C = Ls.conv_C[l];
    if (x.C != p.C) return fail(h, AC_EINVAL, "stream stage %d: %d channels, cache holds %d", l, x.C, p.C);
    if (x.L < p.P) return fail(h, AC_EINVAL, "stream stage %d: %d rows per push, fewer than the %d history rows", l, x.L, p.P);
    if ((size_t)B * (p.P + x.L) * p.C > cap) return fail(h, AC_ENOMEM, "stream stage %d exceeds its workspace buffer", l);
    p.cache = reinterpret_cast<float*>(state + Ls.conv[l]);
    p.x = x.p;
    p.bs = x.bs;
    p.ts = x.ts;
    p.y = staged;
    p.fresh = reinterpret_cast<const int*>(state + Ls.fresh);
    p.B = B;
    p.L = x.L;
    p.replicate = replicate;
    const long long n = (long long)B * (p.P + x.L) * p.C;
    ProfScope ps(h, st, "mstream_stage_kernel", 0.0, 8.0 * n);
    hipLaunchKernelGGL(mstream_stage_kernel, dim3(grid_for(n)), dim3(256), 0, st, p);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

// a causal conv on a staged input: M outputs, output m reads staged rows [m*s, m*s + k) (no padding left)
static int mstream_conv(ac_handle* h, hipStream_t st, const PackedGemm& g, const Act& xs, int k, int s, int M, Out out, int B, Act2* y,
                        const Epi& epi = Epi{}) {
    TapGemmParams p{};
    p.nseg = 1;
    p.seg[0] = make_seg(xs, s, s == 1 ? k : 2, PAD_ZERO, 0, 0, nullptr, 0, 0);
    p.w = h->blob + g.w_off;
    p.bias = g.has_bias ? h->blob + g.b_off : nullptr;
    p.y = out.raw;
    p.y_elu = out.elu;
    p.y_bs = (long long)M * g.N;
    p.y_rs = g.N;
    p.B = B;
    p.M = M;
    p.N = g.N;
    p.Ktot = g.Ktot;
    p.scale = epi.scale;
    p.res = epi.res;
    p.res_bs = epi.res_bs;
    p.res_rs = epi.res_rs;
    const int rc = run_tap(h, st, p);
    if (y) {
        y->raw = Act{out.raw, p.y_bs, p.y_rs, M, g.N, p.amax_out, p.B};
        y->elu = Act{out.elu, p.y_bs, p.y_rs, M, g.N, p.amax_out, p.B};
    }
    return rc;
}

struct MStreamScratch {   // transformer scratch (as mimi_path.hip's TfScratch)
    float *ln, *qkv, *att, *hid;
};

static Act staged_act(const float* p, int B, int rows, int C) { return Act{p, (long long)rows * C, C, rows, C}; }

static void rope_inv(const ac_handle* h, float* inv) {   // mimi_finalize's inv_freq (the host override is gone after finalize)
    const ac_mimi_config& c = h->mcfg;
    for (int j = 0; j < c.head_dim / 2; ++j) inv[j] = 1.0f / std::pow(c.rope_theta, (float)(2 * j) / (float)c.head_dim);
}

// x [B*T][H] in place, as transformer_fwd, with the attention of mstream_attn_kernel
static int mstream_transformer(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, float* x, int B, int T, const MStreamScratch& s) {
    const ac_mimi_config& c = h->mcfg;
    const int H = c.hidden_size, A = Ls.A, I = c.intermediate_size, R = Ls.R;
    const long long rows = (long long)B * T;
    const long long* pos = reinterpret_cast<const long long*>(state + Ls.pos);
    const size_t ring_bytes = align_up((size_t)B * R * A * 4, 256);
    MStreamRopeParams rp{};
    rp.qkv = s.qkv;
    rp.pos = pos;
    rp.B = B;
    rp.T = T;
    rp.A = A;
    rp.HD = c.head_dim;
    rope_inv(h, rp.inv);
    for (size_t l = 0; l < h->mimi.enc_tf.size(); ++l) {
        const MimiTfLayer& L = h->mimi.enc_tf[l];
        float* rk = reinterpret_cast<float*>(state + Ls.ring + (2 * l) * ring_bytes);
        float* rv = reinterpret_cast<float*>(state + Ls.ring + (2 * l + 1) * ring_bytes);
        const unsigned* ln_rows = nullptr;
        int rc = layernorm_fwd(h, st, x, L.ln1_w, L.ln1_b, s.ln, rows, H, c.norm_eps, &ln_rows);
        if (rc) return rc;
        Epi eq;
        eq.rowmax_in = ln_rows;
        if ((rc = mimi_linear(h, st, L.qkv, s.ln, rows, H, H, 0, s.qkv, 3 * A, eq))) return rc;
        {
            const long long n = rows * A;        // (q and k: 2 * heads * HD/2 pairs per row)
            ProfScope ps(h, st, "mstream_rope_kernel", 6.0 * n, 16.0 * n);
            hipLaunchKernelGGL(mstream_rope_kernel, dim3(grid_for(n)), dim3(256), 0, st, rp);
            HIPCHK(h, hipGetLastError());
        }
        {
            MStreamAttnParams ap{s.qkv, rk, rv, pos, s.att, B, T, A, c.head_dim, c.sliding_window, R, 1.0f / std::sqrt((float)c.head_dim)};
            const double keys = std::min<double>(c.sliding_window, T + R);
            ProfScope ps(h, st, "mstream_attn_kernel", 4.0 * rows * A * keys, 8.0 * rows * A * keys);
            hipLaunchKernelGGL(mstream_attn_kernel, dim3(cdiv(T, 4), c.num_attention_heads, B), dim3(256), 0, st, ap);
            HIPCHK(h, hipGetLastError());
        }
        if (R > 0) {   // after the attention: with T >= R the new rows overwrite slots earlier queries of this push still read
            MStreamAppendParams pp{s.qkv, rk, rv, pos, B, T, A, R};
            const long long n = (long long)B * std::min(T, R) * A;
            ProfScope ps(h, st, "mstream_append_kernel", 0.0, 16.0 * n);
            hipLaunchKernelGGL(mstream_append_kernel, dim3(grid_for(n)), dim3(256), 0, st, pp);
            HIPCHK(h, hipGetLastError());
        }
        Epi ea;
        ea.scale = h->blob + L.sc_a;
        ea.res = x;
        ea.res_rs = H;
        if ((rc = mimi_linear(h, st, L.o, s.att, rows, A, A, 0, x, H, ea))) return rc;
        if ((rc = layernorm_fwd(h, st, x, L.ln2_w, L.ln2_b, s.ln, rows, H, c.norm_eps, &ln_rows))) return rc;
        Epi eg;
        eg.gelu = 1;
        eg.rowmax_in = ln_rows;
        const unsigned* hid_rows = nullptr;
        eg.rowmax_out = &hid_rows;
        if ((rc = mimi_linear(h, st, L.fc1, s.ln, rows, H, H, 0, s.hid, I, eg))) return rc;
        Epi em;
        em.rowmax_in = hid_rows;
        em.scale = h->blob + L.sc_m;
        em.res = x;
        em.res_rs = H;
        if ((rc = mimi_linear(h, st, L.fc2, s.hid, rows, I, I, 0, x, H, em))) return rc;
    }
    return AC_OK;
}

// one push: sig [B][F*hop] -> feats [B][F][H]; the stream state advances by F frames
static int mstream_encoder(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, const float* sig, int B, int F, float* feats,
                           WsPtrs& ws, size_t cap) {
    const ac_mimi_config& c = h->mcfg;
    const MimiPlan& m = h->mimi;
    const int T = F * h->hop;
    int l = 0, rc;
    Act2 x, y;
    float* stg = ws.take();
    if ((rc = mstream_stage(h, st, state, Ls, l, Act{sig, (long long)T, 1, T, 1}, B, stg, cap, false))) return rc;
    if ((rc = mstream_conv(h, st, m.enc_stem, staged_act(stg, B, T + Ls.conv_P[l], 1), c.kernel_size, 1, T, Out{ws.take(), ws.take()}, B, &x))) return rc;
    ws.give(stg);
    ++l;
    for (int i = 0; i < c.num_ratios; ++i) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - i];
        const ResBlockPlan& rb = m.enc_rb[i];
        const int L = x.raw.L, ch = rb.C;
        // residual block: x + conv_k1(ELU(conv_k3(ELU(x)))), the k3 conv on [history | ELU(x)]
        stg = ws.take();
        if ((rc = mstream_stage(h, st, state, Ls, l, x.elu, B, stg, cap, false))) return rc;
        ws.give(x.elu.p);
        float* hb = ws.take();
        Act2 hv;
        if ((rc = mstream_conv(h, st, rb.c3, staged_act(stg, B, L + Ls.conv_P[l], ch), c.residual_kernel_size, 1, L, Out{nullptr, hb}, B, &hv))) return rc;
        ws.give(stg);
        ++l;
        Epi e;
        e.res = x.raw.p;
        e.res_bs = x.raw.bs;
        e.res_rs = x.raw.ts;
        if ((rc = mstream_conv(h, st, rb.fused, hv.elu, 1, 1, L, Out{ws.take(), ws.take()}, B, &y, e))) return rc;
        ws.give(hb);
        ws.give(x.raw.p);
        x = y;
        // down-sampler (k = 2 * ratio, stride ratio) on [history | ELU(x)]
        stg = ws.take();
        if ((rc = mstream_stage(h, st, state, Ls, l, x.elu, B, stg, cap, false))) return rc;
        ws.give(x);
        const bool last = i == c.num_ratios - 1;     // the last one feeds ELU -> final conv only
        if ((rc = mstream_conv(h, st, m.enc_down[i], staged_act(stg, B, L + Ls.conv_P[l], ch), 2 * ratio, ratio, L / ratio,
                               Out{last ? nullptr : ws.take(), ws.take()}, B, &x)))
            return rc;
        ws.give(stg);
        ++l;
    }
    const int T25 = x.elu.L;
    stg = ws.take();
    if ((rc = mstream_stage(h, st, state, Ls, l, x.elu, B, stg, cap, false))) return rc;
    ws.give(x);
    float* stream = ws.take();
    if ((rc = mstream_conv(h, st, m.enc_final, staged_act(stg, B, T25 + Ls.conv_P[l], m.D), c.last_kernel_size, 1, T25, Out{stream, nullptr}, B, nullptr))) return rc;
    ws.give(stg);
    ++l;
    MStreamScratch s{ws.take(), ws.take(), ws.take(), ws.take()};
    if ((rc = mstream_transformer(h, st, state, Ls, stream, B, T25, s))) return rc;
    ws.give(s.ln); ws.give(s.qkv); ws.give(s.att); ws.give(s.hid);
    stg = ws.take();
    const int H = c.hidden_size;
    if ((rc = mstream_stage(h, st, state, Ls, l, Act{stream, (long long)T25 * H, H, T25, H}, B, stg, cap, true))) return rc;
    ws.give(stream);
    if ((rc = mstream_conv(h, st, m.down, staged_act(stg, B, T25 + Ls.conv_P[l], H), 2 * c.resample_stride, c.resample_stride, F,
                           Out{feats, nullptr}, B, nullptr)))
        return rc;
    ws.give(stg);
    hipLaunchKernelGGL(mstream_advance_kernel, dim3(cdiv(B, 64)), dim3(64), 0, st, reinterpret_cast<long long*>(state + Ls.pos),
                       reinterpret_cast<int*>(state + Ls.fresh), B, T25);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

static Workspace mstream_plan_ws(const ac_handle* h, int B, int F) {
    // the batch plan for one frame more than the push: every level gets hop / (its stride) >= k - stride spare rows for its history
    return mimi_plan_ws(h, B, (F + 1) * h->hop, 0, true);
}

static int mstream_check(ac_handle* h, int B) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->arch != ARCH_MIMI) return fail(h, AC_EINVAL, "ac_mimi_stream: not a Mimi handle");
    if (!h->has_enc) return fail(h, AC_ESTATE, "ac_mimi_stream: the handle was loaded without encoder weights (mode=\"decode\")");
    if (B < 1) return fail(h, AC_EINVAL, "ac_mimi_stream: B=%d", B);
    if (h->mcfg.head_dim > MSTREAM_MAXHD) return fail(h, AC_EINVAL, "ac_mimi_stream: head_dim %d unsupported", h->mcfg.head_dim);
    return AC_OK;
}

}  // namespace acimpl

using namespace acimpl;

extern "C" {

size_t ac_mimi_stream_state_bytes(const ac_handle* h, int B) {
    if (!h || B < 1 || h->arch != ARCH_MIMI) return 0;
    return mstream_layout(h, B).total;
}

size_t ac_mimi_stream_workspace_bytes(const ac_handle* h, int B, int F) {
    if (!h || B < 1 || F < 1 || h->arch != ARCH_MIMI) return 0;
    return mstream_plan_ws(h, B, F).total_bytes;
}

int ac_mimi_stream_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream) {
    int rc = mstream_check(h, B);
    if (rc) return rc;
    if (!state_dev) return fail(h, AC_EINVAL, "ac_mimi_stream_reset: state is null");
    const MStreamLayout Ls = mstream_layout(h, B);
    if (state_bytes < Ls.total) return fail(h, AC_ENOMEM, "ac_mimi_stream_reset: state of %zu bytes, %zu needed", state_bytes, Ls.total);
    if ((reinterpret_cast<uintptr_t>(state_dev) & 255) != 0) return fail(h, AC_EINVAL, "ac_mimi_stream_reset: state must be 256-byte aligned");
    auto it = h->mimi_streams.find(state_dev);
    if (reset_mask_dev && (it == h->mimi_streams.end() || it->second != B))
        return fail(h, AC_EINVAL, "ac_mimi_stream_reset: a masked reset needs a state this handle reset for B=%d before", B);
    char* s = static_cast<char*>(state_dev);
    MStreamHeader hd{MSTREAM_MAGIC, 1u, mstream_fingerprint(h->mcfg), B, 0};
    hipLaunchKernelGGL(mstream_reset_kernel, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<MStreamHeader*>(s), hd,
                       reinterpret_cast<long long*>(s + Ls.pos), reinterpret_cast<int*>(s + Ls.fresh), reset_mask_dev, B);
    HIPCHK(h, hipGetLastError());
    h->mimi_streams[state_dev] = B;
    return AC_OK;
}

int ac_mimi_stream_encode(ac_handle* h, void* state_dev, size_t state_bytes, const float* sig_dev, int B, int F, int K, int64_t* toks_dev,
                          void* ws, size_t ws_bytes, void* stream) {
    int rc = mstream_check(h, B);
    if (rc) return rc;
    if (!state_dev || !sig_dev || !toks_dev || F < 1) return fail(h, AC_EINVAL, "ac_mimi_stream_encode: bad argument (F=%d)", F);
    if (K < 1 || K > h->mcfg.num_quantizers) return fail(h, AC_EINVAL, "ac_mimi_stream_encode: K=%d outside [1, %d]", K, h->mcfg.num_quantizers);
    auto it = h->mimi_streams.find(state_dev);
    if (it == h->mimi_streams.end()) return fail(h, AC_EINVAL, "ac_mimi_stream_encode: the state was never reset on this handle");
    if (it->second != B) return fail(h, AC_EINVAL, "ac_mimi_stream_encode: the state holds %d streams, B=%d", it->second, B);
    const MStreamLayout Ls = mstream_layout(h, B);
    if (state_bytes < Ls.total) return fail(h, AC_ENOMEM, "ac_mimi_stream_encode: state of %zu bytes, %zu needed", state_bytes, Ls.total);
    if ((long long)F * h->hop > 0x7fffffffLL / 64) return fail(h, AC_EINVAL, "ac_mimi_stream_encode: F=%d frames per push is too many", F);
    const Workspace w = mstream_plan_ws(h, B, F);
    WsPtrs p;
    if ((rc = carve(h, w, ws, ws_bytes, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = amax_begin(h, st, B))) return rc;
    const ac_mimi_config& c = h->mcfg;
    float* feats = p.act[NACT - 1];   // the push never has more than 5 buffers live
    p.used[NACT - 1] = true;
    rc = mstream_encoder(h, st, static_cast<char*>(state_dev), Ls, sig_dev, B, F, feats, p, w.act_floats);
    if (rc) return rc;
    float* proj = p.take();
    rc = mimi_linear(h, st, h->mimi.in_proj, feats, (long long)B * F, c.hidden_size, c.hidden_size, 0, proj, 2 * c.codebook_dim);
    if (rc) return rc;
    return mimi_rvq_encode(h, st, proj, B * F, K, reinterpret_cast<long long*>(toks_dev));
}

}  // extern "C"
