// Streaming Mimi encode (include/audiocodecs_amd.h ac_mimi_stream_*; DESIGN.md "Streaming Mimi encode").
// A push of F whole frames per stream runs the batch encoder's layers on [history | chunk]: every causal conv reads its last
// k - stride input rows from the stream state (mstream_stage_kernel, then the tap-GEMM with no left padding); the transformer's
// attention reads the K / V ring of the previous sliding_window - 1 positions (mstream_attn_kernel).  The fused batch-only blocks
// (rb_stream6m with the folded stem, rb_stream128m, rb_fused6) assume zero history: a push goes through the per-conv tap-GEMMs.
// The caller owns the state and the workspace; no entry point here allocates or synchronises.
//
// Streaming Mimi decode (ac_mimi_stream_decode*; DESIGN.md "Streaming Mimi decode") is the mirror image: a push of F token frames runs
// the batch decoder's layers on [history | chunk] -- the up-sampler's previous input row, the decoder transformer's K / V rings
// (positions advance resample_stride per frame), the first conv's k - 1 rows, each transposed conv's previous input row (with
// k = 2 stride it is convtr_fwd's 2-tap row conv, its left zero row replaced by the cached one), each residual block's k3 history
// and the head conv's.  A decode state has its own layout and magic and is registered separately on the handle.  The transformer's
// linear layers of a push with few rows go through mstream_linear_kernel (stream_stage.h) instead of the tap-GEMM.
//
// Slot pushes (ac_mimi_stream_encode_slots / _decode_slots) run n listed streams of the B a state holds: the same
// launch sequence on n dense rows, with the conv caches, the positions and the K / V rings addressed through the caller's slot list.
#include "core.h"
#include "stream_launch.h"
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
    int B = 0;                                 // streams the state holds
};

static MStreamLayout mstream_layout(const ac_handle* h, int B) {
    const ac_mimi_config& c = h->mcfg;
    MStreamLayout L;
    L.B = B;
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

// decode state: the caches in decoder order -- up-sampler input, first conv, (transposed conv input, block k3) per ratio, head conv
static MStreamLayout mdstream_layout(const ac_handle* h, int B) {
    const ac_mimi_config& c = h->mcfg;
    MStreamLayout L;
    L.B = B;
    size_t off = align_up(sizeof(MStreamHeader), 256);
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    L.pos = take((size_t)B * 8);
    L.fresh = take((size_t)B * 4);
    auto conv = [&](int P, int C) { L.conv.push_back(take((size_t)B * std::max(P, 1) * C * 4)); L.conv_P.push_back(P); L.conv_C.push_back(C); };
    conv(1, c.hidden_size);
    conv(c.kernel_size - 1, c.hidden_size);
    int ch = h->mimi.D;
    for (int i = 0; i < c.num_ratios; ++i) {
        conv(1, ch);
        ch /= 2;
        conv(c.residual_kernel_size - 1, ch);
    }
    conv(c.last_kernel_size - 1, ch);
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

// [cache | x] -> staged, x's last P rows -> cache (stream_launch.h), on cache `l` of the state.
// (`slot`, here and below: the slot map of a push that runs B listed streams of the state's Ls.B -- stream_stage.h; null = all, in order)
static int mstream_stage(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, const int* slot, int l, const Act& x, int B, float* staged,
                         size_t cap, bool replicate, bool any_L = false) {
    return stream_stage(h, st, reinterpret_cast<float*>(state + Ls.conv[l]), reinterpret_cast<const int*>(state + Ls.fresh), Ls.conv_P[l], Ls.conv_C[l], l, x, B,
                        staged, cap, replicate ? STAGE_REPLICATE : STAGE_ZERO, any_L, slot, Ls.B);
}

struct MStreamScratch {   // transformer scratch (as mimi_path.hip's TfScratch)
    float *ln, *qkv, *att, *hid;
};

static void rope_inv(const ac_handle* h, float* inv) {   // mimi_finalize's inv_freq (the host override is gone after finalize)
    const ac_mimi_config& c = h->mcfg;
    for (int j = 0; j < c.head_dim / 2; ++j) inv[j] = 1.0f / std::pow(c.rope_theta, (float)(2 * j) / (float)c.head_dim);
}

// Rows per launch (B * T) up to which the decode stream's linear layers take mstream_linear_kernel when the switch "mstream_skinny" is
// on auto (-1).  Source: profiles/mimi_dstream_latency.jsonl (one MI355X, tools/mimi_stream_latency.py --direction decode
// --linear-route ab, 200 pushes per route, median push latency tap-GEMM / skinny in ms): 2 rows 3.24 / 1.91, 8 rows 3.32 / 2.10,
// 32 rows 3.76 / 2.53, 128 rows 4.33 / 3.48, 256 rows 5.34 / 5.12, 1280 rows 9.08 / 13.65.  128 is the largest measured point where the
// skinny route wins by far more than the A/B's run-to-run spread (0.02 ms at 2 rows, p99 - median up to 0.3 ms); at 256 the two meet.
constexpr int MSTREAM_SKINNY_AUTO_ROWS = 128;

static bool mstream_skinny_ok(const PackedGemm& g, const float* x, int x_pitch, const float* y, int y_pitch, int K) {
    return !g.has_bias && K == g.Ktot && K % 4 == 0 && (K / mstream_linear_ks(K)) % 4 == 0 && x_pitch % 4 == 0 && aligned16(x) && (g.w_off % 4) == 0 && y && y_pitch >= g.N;
}

template <int RB>
static void mstream_linear_launch(hipStream_t st, const MStreamLinearParams& p) {
    const dim3 grid((unsigned)p.N, (unsigned)cdiv(p.R, RB));
    if (mstream_linear_ks(p.K) == 4) hipLaunchKernelGGL((mstream_linear_kernel<RB, 4>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((mstream_linear_kernel<RB, 1>), grid, dim3(64), 0, st, p);
}

// y[rows][N] = epi(x[rows][K] W^T) as linear_rows computes it, on the plain fp32 matrix; shapes the kernel does not take go to linear_rows
static int mstream_linear(ac_handle* h, hipStream_t st, const PackedGemm& g, const float* x, long long rows, int K, float* y, int y_pitch, const Epi& epi, bool skinny) {
    if (!skinny || rows > 65535LL * 8 || !mstream_skinny_ok(g, x, K, y, y_pitch, K)) return linear_rows(h, st, g, x, rows, K, K, 0, y, y_pitch, epi);
    MStreamLinearParams p{};
    p.x = x;
    p.w = h->blob + g.w_off;
    p.y = y;
    p.scale = epi.scale;
    p.res = epi.res;
    p.x_pitch = K;
    p.y_pitch = y_pitch;
    p.res_pitch = (int)epi.res_rs;
    p.R = (int)rows;
    p.N = g.N;
    p.K = K;
    p.gelu = epi.gelu;
    if (epi.rowmax_out) *epi.rowmax_out = nullptr;
    ProfScope ps(h, st, "mstream_linear_kernel", 2.0 * rows * g.N * K, 4.0 * ((double)g.N * K + (double)rows * (K + g.N)));
    if (rows <= 2) mstream_linear_launch<2>(st, p);
    else if (rows <= 4) mstream_linear_launch<4>(st, p);
    else mstream_linear_launch<8>(st, p);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

// x [B*T][H] in place, as transformer_fwd, with the attention of mstream_attn_kernel.  `skinny`: the linear layers through
// mstream_linear (the decode stream's choice; the encode stream passes false and keeps the tap-GEMM route bit for bit).
// B is the dense row count of the push: every activation is [B][T]; only the positions and the rings ([Ls.B] streams) go through `slot`.
// Test hook (ac_debug_capture): per layer the rotated qkv, the attention's output and the layer's output, as stream-ordered copies.
static int mstream_transformer(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, const int* slot, const std::vector<MimiTfLayer>& layers,
                               bool skinny, float* x, int B, int T, const MStreamScratch& s) {
    const ac_mimi_config& c = h->mcfg;
    const int H = c.hidden_size, A = Ls.A, I = c.intermediate_size, R = Ls.R;
    const long long rows = (long long)B * T;
    const long long* pos = reinterpret_cast<const long long*>(state + Ls.pos);
    const size_t ring_bytes = align_up((size_t)Ls.B * R * A * 4, 256);
    MStreamRopeParams rp{};
    rp.qkv = s.qkv;
    rp.pos = pos;
    rp.B = B;
    rp.T = T;
    rp.A = A;
    rp.HD = c.head_dim;
    rope_inv(h, rp.inv);
    rp.slot = slot;
    rp.cap = Ls.B;
    for (size_t l = 0; l < layers.size(); ++l) {
        const MimiTfLayer& L = layers[l];
        float* rk = reinterpret_cast<float*>(state + Ls.ring + (2 * l) * ring_bytes);
        float* rv = reinterpret_cast<float*>(state + Ls.ring + (2 * l + 1) * ring_bytes);
        const unsigned* ln_rows = nullptr;
        int rc = layernorm_fwd(h, st, x, L.ln1_w, L.ln1_b, s.ln, rows, H, c.norm_eps, skinny ? nullptr : &ln_rows);   // (row words: the split16 route's)
        if (rc) return rc;
        Epi eq;
        eq.rowmax_in = ln_rows;
        if ((rc = mstream_linear(h, st, L.qkv, s.ln, rows, H, s.qkv, 3 * A, eq, skinny))) return rc;
        {
            const long long n = rows * A;        // (q and k: 2 * heads * HD/2 pairs per row)
            ProfScope ps(h, st, "mstream_rope_kernel", 6.0 * n, 16.0 * n);
            hipLaunchKernelGGL(mstream_rope_kernel, dim3(grid_for(n)), dim3(256), 0, st, rp);
            HIPCHK(h, hipGetLastError());
        }
        capture(h, st, Act{s.qkv, (long long)T * 3 * A, 3 * A, T, 3 * A}, B);
        {
            MStreamAttnParams ap{s.qkv, rk, rv, pos, s.att, B, T, A, c.head_dim, c.sliding_window, R, 1.0f / std::sqrt((float)c.head_dim), slot, Ls.B};
            const double keys = std::min<double>(c.sliding_window, T + R);
            ProfScope ps(h, st, "mstream_attn_kernel", 4.0 * rows * A * keys, 8.0 * rows * A * keys);
            hipLaunchKernelGGL(mstream_attn_kernel, dim3(cdiv(T, 4), c.num_attention_heads, B), dim3(256), 0, st, ap);
            HIPCHK(h, hipGetLastError());
        }
        capture(h, st, Act{s.att, (long long)T * A, A, T, A}, B);
        if (R > 0) {   // after the attention: with T >= R the new rows overwrite slots earlier queries of this push still read
            MStreamAppendParams pp{s.qkv, rk, rv, pos, B, T, A, R, slot, Ls.B};
            const long long n = (long long)B * std::min(T, R) * A;
            ProfScope ps(h, st, "mstream_append_kernel", 0.0, 16.0 * n);
            hipLaunchKernelGGL(mstream_append_kernel, dim3(grid_for(n)), dim3(256), 0, st, pp);
            HIPCHK(h, hipGetLastError());
        }
        Epi ea;
        ea.scale = h->blob + L.sc_a;
        ea.res = x;
        ea.res_rs = H;
        if ((rc = mstream_linear(h, st, L.o, s.att, rows, A, x, H, ea, skinny))) return rc;
        if ((rc = layernorm_fwd(h, st, x, L.ln2_w, L.ln2_b, s.ln, rows, H, c.norm_eps, skinny ? nullptr : &ln_rows))) return rc;
        Epi eg;
        eg.gelu = 1;
        eg.rowmax_in = ln_rows;
        const unsigned* hid_rows = nullptr;
        if (!skinny) eg.rowmax_out = &hid_rows;
        if ((rc = mstream_linear(h, st, L.fc1, s.ln, rows, H, s.hid, I, eg, skinny))) return rc;
        Epi em;
        em.rowmax_in = hid_rows;
        em.scale = h->blob + L.sc_m;
        em.res = x;
        em.res_rs = H;
        if ((rc = mstream_linear(h, st, L.fc2, s.hid, rows, I, x, H, em, skinny))) return rc;
        capture(h, st, Act{x, (long long)T * H, H, T, H}, B);
    }
    return AC_OK;
}

// one push: sig [B][F*hop] -> feats [B][F][H]; the stream state advances by F frames
static int mstream_encoder(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, const int* slot, const float* sig, int B, int F, float* feats,
                           WsPtrs& ws, size_t cap) {
    const ac_mimi_config& c = h->mcfg;
    const MimiPlan& m = h->mimi;
    const int T = F * h->hop;
    int l = 0, rc;
    Act2 x, y;
    float* stg = ws.take();
    if ((rc = mstream_stage(h, st, state, Ls, slot, l, Act{sig, (long long)T, 1, T, 1}, B, stg, cap, false))) return rc;
    if ((rc = mstream_conv(h, st, m.enc_stem, staged_act(stg, B, T + Ls.conv_P[l], 1), c.kernel_size, 1, T, Out{ws.take(), ws.take()}, B, &x))) return rc;
    ws.give(stg);
    ++l;
    for (int i = 0; i < c.num_ratios; ++i) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - i];
        const ResBlockPlan& rb = m.enc_rb[i];
        const int L = x.raw.L, ch = rb.C;
        // residual block: x + conv_k1(ELU(conv_k3(ELU(x)))), the k3 conv on [history | ELU(x)]
        stg = ws.take();
        if ((rc = mstream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, false))) return rc;
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
        if ((rc = mstream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, false))) return rc;
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
    if ((rc = mstream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, false))) return rc;
    ws.give(x);
    float* stream = ws.take();
    if ((rc = mstream_conv(h, st, m.enc_final, staged_act(stg, B, T25 + Ls.conv_P[l], m.D), c.last_kernel_size, 1, T25, Out{stream, nullptr}, B, nullptr))) return rc;
    ws.give(stg);
    ++l;
    capture(h, st, Act{stream, (long long)T25 * c.hidden_size, c.hidden_size, T25, c.hidden_size}, B);   // test hook: the transformer's input
    MStreamScratch s{ws.take(), ws.take(), ws.take(), ws.take()};
    if ((rc = mstream_transformer(h, st, state, Ls, slot, m.enc_tf, false, stream, B, T25, s))) return rc;
    ws.give(s.ln); ws.give(s.qkv); ws.give(s.att); ws.give(s.hid);
    stg = ws.take();
    const int H = c.hidden_size;
    if ((rc = mstream_stage(h, st, state, Ls, slot, l, Act{stream, (long long)T25 * H, H, T25, H}, B, stg, cap, true))) return rc;
    ws.give(stream);
    if ((rc = mstream_conv(h, st, m.down, staged_act(stg, B, T25 + Ls.conv_P[l], H), 2 * c.resample_stride, c.resample_stride, F,
                           Out{feats, nullptr}, B, nullptr)))
        return rc;
    ws.give(stg);
    hipLaunchKernelGGL(mstream_advance_kernel<>, dim3(cdiv(B, 64)), dim3(64), 0, st, reinterpret_cast<long long*>(state + Ls.pos),
                       reinterpret_cast<int*>(state + Ls.fresh), B, T25, slot, Ls.B);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

// one push: toks [B][F][K] -> sig [B][F*hop]; the decode state advances by F frames (mimi_decoder_fwd on [history | chunk])
static int mstream_decoder(ac_handle* h, hipStream_t st, char* state, const MStreamLayout& Ls, const int* slot, const long long* toks, int B, int F, int K, float* sig,
                           WsPtrs& ws, size_t cap, bool skinny) {
    const ac_mimi_config& c = h->mcfg;
    const MimiPlan& m = h->mimi;
    const int H = c.hidden_size, rs = c.resample_stride, T25 = F * rs;
    int l = 0, rc;
    float* qsum = ws.take();
    float* qf = ws.take();
    if ((rc = mimi_rvq_decode(h, st, toks, B * F, K, qsum, qf))) return rc;
    ws.give(qsum);
    capture(h, st, Act{qf, (long long)F * H, H, F, H}, B);   // test hook: the dequantised rows
    // up-sampler: depthwise transposed conv (k = 2 stride) on [previous input row | chunk]
    float* stg = ws.take();
    if ((rc = mstream_stage(h, st, state, Ls, slot, l, Act{qf, (long long)F * H, H, F, H}, B, stg, cap, false, true))) return rc;
    ws.give(qf);
    ++l;
    float* stream = ws.take();
    if ((size_t)B * T25 * H > cap) return fail(h, AC_ENOMEM, "stream up-sampler exceeds its workspace buffer");
    {
        MStreamUpsampleParams p{stg, h->blob + m.up_w, stream, B, F, H, rs};
        const long long total = (long long)B * T25 * (H / 4);
        ProfScope ps(h, st, "mstream_upsample_kernel", 4.0 * B * (double)T25 * H, 4.0 * B * (double)H * (F + 1 + T25));
        hipLaunchKernelGGL(mstream_upsample_kernel, dim3(grid_for(total)), dim3(256), 0, st, p);
        HIPCHK(h, hipGetLastError());
    }
    ws.give(stg);
    capture(h, st, Act{stream, (long long)T25 * H, H, T25, H}, B);   // test hook: the up-sampler's output, the transformer's input
    MStreamScratch s{ws.take(), ws.take(), ws.take(), ws.take()};
    if ((rc = mstream_transformer(h, st, state, Ls, slot, m.dec_tf, skinny, stream, B, T25, s))) return rc;
    ws.give(s.ln); ws.give(s.qkv); ws.give(s.att); ws.give(s.hid);
    // first conv (k7) on [history | chunk]: a one-frame push brings fewer rows than the history holds
    Act2 x, y;
    stg = ws.take();
    if ((rc = mstream_stage(h, st, state, Ls, slot, l, Act{stream, (long long)T25 * H, H, T25, H}, B, stg, cap, false, true))) return rc;
    ws.give(stream);
    if ((rc = mstream_conv(h, st, m.dec_first, staged_act(stg, B, T25 + Ls.conv_P[l], H), c.kernel_size, 1, T25, Out{nullptr, ws.take()}, B, &x))) return rc;
    ws.give(stg);
    ++l;
    for (int i = 0; i < c.num_ratios; ++i) {
        const int ratio = c.upsampling_ratios[i], cin = m.dec_up[i].Ktot / 2, cup = m.dec_up[i].N / ratio, L = x.elu.L;
        // transposed conv (k = 2 ratio): output row m = [x[m-1] | x[m]] Wp (convtr_fwd), x[-1] from the cache
        stg = ws.take();
        if ((rc = mstream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, false, true))) return rc;
        ws.give(x);
        if ((rc = mstream_conv(h, st, m.dec_up[i], staged_act(stg, B, L + Ls.conv_P[l], cin), 2, 1, L, Out{ws.take(), ws.take()}, B, &y))) return rc;
        ws.give(stg);
        ++l;
        const int Lu = L * ratio;                      // [B][L][ratio * cup] is [B][L * ratio][cup]
        x.raw = Act{y.raw.p, (long long)Lu * cup, cup, Lu, cup, y.raw.amax, y.raw.amax_n};
        x.elu = Act{y.elu.p, (long long)Lu * cup, cup, Lu, cup, y.elu.amax, y.elu.amax_n};
        // residual block: x + conv_k1(ELU(conv_k3(ELU(x)))), the k3 conv on [history | ELU(x)]
        const ResBlockPlan& rb = m.dec_rb[i];
        stg = ws.take();
        if ((rc = mstream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, false, true))) return rc;
        ws.give(x.elu.p);
        float* hb = ws.take();
        Act2 hv;
        if ((rc = mstream_conv(h, st, rb.c3, staged_act(stg, B, Lu + Ls.conv_P[l], cup), c.residual_kernel_size, 1, Lu, Out{nullptr, hb}, B, &hv))) return rc;
        ws.give(stg);
        ++l;
        Epi e;
        e.res = x.raw.p;
        e.res_bs = x.raw.bs;
        e.res_rs = x.raw.ts;
        const bool last = i == c.num_ratios - 1;       // the head conv reads ELU(y) only
        if ((rc = mstream_conv(h, st, rb.fused, hv.elu, 1, 1, Lu, Out{last ? nullptr : ws.take(), ws.take()}, B, &y, e))) return rc;
        ws.give(hb);
        ws.give(x.raw.p);
        x = y;
    }
    const int Ts = x.elu.L, Fh = c.num_filters;
    stg = ws.take();
    if ((rc = mstream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, false, true))) return rc;
    ws.give(x);
    if ((rc = mstream_conv(h, st, m.dec_head, staged_act(stg, B, Ts + Ls.conv_P[l], Fh), c.last_kernel_size, 1, Ts, Out{sig, nullptr}, B, nullptr))) return rc;
    ws.give(stg);
    hipLaunchKernelGGL(mstream_advance_kernel<>, dim3(cdiv(B, 64)), dim3(64), 0, st, reinterpret_cast<long long*>(state + Ls.pos),
                       reinterpret_cast<int*>(state + Ls.fresh), B, T25, slot, Ls.B);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

static Workspace mdstream_plan_ws(const ac_handle* h, int B, int F) {
    // the batch plan for four frames more than the push: 4 * resample_stride >= kernel_size - 1 spare rows for the first conv's staged
    // input (ac_mimi_create: kernel_size <= 8, resample_stride >= 1 -- two or more in every real model), and more than that at every later level
    return mimi_plan_ws(h, B, 0, F + 4 + (h->mcfg.resample_stride == 1 ? 4 : 0), false);
}

static Workspace mstream_plan_ws(const ac_handle* h, int B, int F) {
    // the batch plan for one frame more than the push: every level gets hop / (its stride) >= k - stride spare rows for its history
    return mimi_plan_ws(h, B, (F + 1) * h->hop, 0, true);
}

static int mstream_check(ac_handle* h, int B, bool dec = false) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->arch != ARCH_MIMI) return fail(h, AC_EINVAL, "ac_mimi_stream: not a Mimi handle");
    if (!dec && !h->has_enc) return fail(h, AC_ESTATE, "ac_mimi_stream: the handle was loaded without encoder weights (mode=\"decode\")");
    if (dec && !h->has_dec) return fail(h, AC_ESTATE, "ac_mimi_stream_decode: the handle was loaded without decoder weights (mode=\"encode\")");
    if (B < 1) return fail(h, AC_EINVAL, "ac_mimi_stream: B=%d", B);
    if (h->mcfg.head_dim > MSTREAM_MAXHD) return fail(h, AC_EINVAL, "ac_mimi_stream: head_dim %d unsupported", h->mcfg.head_dim);
    return AC_OK;
}

// The checks of a push that touch nothing, in the order both directions make them; *Ls: the state's layout.
static int mstream_push_check(ac_handle* h, void* state_dev, size_t state_bytes, const void* in, const void* out, int B, const int* slots_host, int n,
                              int F, int K, bool dec, const char* who, MStreamLayout* Ls) {
    int rc = mstream_check(h, B, dec);
    if (rc) return rc;
    if (!state_dev || !in || !out || F < 1) return fail(h, AC_EINVAL, "%s: bad argument (F=%d)", who, F);
    if (K < 1 || K > h->mcfg.num_quantizers) return fail(h, AC_EINVAL, "%s: K=%d outside [1, %d]", who, K, h->mcfg.num_quantizers);
    const auto& mine = dec ? h->mimi_dstreams : h->mimi_streams;
    const auto& other = dec ? h->mimi_streams : h->mimi_dstreams;
    auto it = mine.find(state_dev);
    if (it == mine.end())
        return fail(h, AC_EINVAL, "%s: the state was never reset%s on this handle%s", who, dec ? " as a decode state" : "",
                    !other.count(state_dev) ? "" : dec ? " (it is an encode state)" : " as an encode state (it is a decode state)");
    if (it->second != B) return fail(h, AC_EINVAL, "%s: the state holds %d streams, B=%d", who, it->second, B);
    *Ls = dec ? mdstream_layout(h, B) : mstream_layout(h, B);
    if (state_bytes < Ls->total) return fail(h, AC_ENOMEM, "%s: state of %zu bytes, %zu needed", who, state_bytes, Ls->total);
    if ((long long)F * h->hop > 0x7fffffffLL / 64) return fail(h, AC_EINVAL, "%s: F=%d frames per push is too many", who, F);
    if (slots_host && (rc = stream_slots_check(h, slots_host, n, B, who))) return rc;
    return AC_OK;
}

// One push of n streams of a state of B: all of them in order (a lockstep push: slots_host = slots_dev = null, n = B) or the listed
// ones.  Every buffer, scale and launch shape is that of a dense push of n streams; `slots_dev` only redirects the addresses into the
// state.  Mimi pads with zeros: a fresh stream takes any F >= 1, and the host keeps no per-slot record.
static int mstream_encode(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                          const float* sig_dev, int F, int K, int64_t* toks_dev, void* ws, size_t ws_bytes, void* stream, const char* who) {
    MStreamLayout Ls;
    int rc = mstream_push_check(h, state_dev, state_bytes, sig_dev, toks_dev, B, slots_host, n, F, K, false, who, &Ls);
    if (rc) return rc;
    const Workspace w = mstream_plan_ws(h, n, F);
    WsPtrs p;
    if ((rc = carve(h, w, ws, ws_bytes, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = amax_begin(h, st, n))) return rc;
    const ac_mimi_config& c = h->mcfg;
    float* feats = p.act[NACT - 1];   // the push never has more than 5 buffers live
    p.used[NACT - 1] = true;
    rc = mstream_encoder(h, st, static_cast<char*>(state_dev), Ls, slots_dev, sig_dev, n, F, feats, p, w.act_floats);
    if (rc) return rc;
    float* proj = p.take();
    rc = linear_rows(h, st, h->mimi.in_proj, feats, (long long)n * F, c.hidden_size, c.hidden_size, 0, proj, 2 * c.codebook_dim);
    if (rc) return rc;
    return mimi_rvq_encode(h, st, proj, n * F, K, reinterpret_cast<long long*>(toks_dev));
}

static int mstream_decode(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                          const int64_t* toks_dev, int F, int K, float* sig_dev, void* ws, size_t ws_bytes, void* stream, const char* who) {
    MStreamLayout Ls;
    int rc = mstream_push_check(h, state_dev, state_bytes, toks_dev, sig_dev, B, slots_host, n, F, K, true, who, &Ls);
    if (rc) return rc;
    const Workspace w = mdstream_plan_ws(h, n, F);
    WsPtrs p;
    if ((rc = carve(h, w, ws, ws_bytes, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = amax_begin(h, st, n))) return rc;
    const long long rows = (long long)n * F * h->mcfg.resample_stride;      // rows of one linear-layer launch (dense: the listed streams)
    const int sw = h->dev.mstream_skinny;
    const bool skinny = sw > 0 || (sw < 0 && rows <= MSTREAM_SKINNY_AUTO_ROWS);
    return mstream_decoder(h, st, static_cast<char*>(state_dev), Ls, slots_dev, reinterpret_cast<const long long*>(toks_dev), n, F, K, sig_dev, p, w.act_floats, skinny);
}

// ac_mimi_stream_reset / _decode_reset: the header, and position = 0, fresh = 1 for every stream or the masked ones
static int mstream_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream, bool dec) {
    const char* who = dec ? "ac_mimi_stream_decode_reset" : "ac_mimi_stream_reset";
    int rc = mstream_check(h, B, dec);
    if (rc) return rc;
    if (!state_dev) return fail(h, AC_EINVAL, "%s: state is null", who);
    const MStreamLayout Ls = dec ? mdstream_layout(h, B) : mstream_layout(h, B);
    if (state_bytes < Ls.total) return fail(h, AC_ENOMEM, "%s: state of %zu bytes, %zu needed", who, state_bytes, Ls.total);
    if ((reinterpret_cast<uintptr_t>(state_dev) & 255) != 0) return fail(h, AC_EINVAL, "%s: state must be 256-byte aligned", who);
    auto& mine = dec ? h->mimi_dstreams : h->mimi_streams;
    auto it = mine.find(state_dev);
    if (reset_mask_dev && (it == mine.end() || it->second != B))
        return fail(h, AC_EINVAL, "%s: a masked reset needs a %sstate this handle reset for B=%d before", who, dec ? "decode " : "", B);
    char* s = static_cast<char*>(state_dev);
    MStreamHeader hd{dec ? MDSTREAM_MAGIC : MSTREAM_MAGIC, 1u, mstream_fingerprint(h->mcfg), B, 0};
    hipLaunchKernelGGL(mstream_reset_kernel<>, dim3(cdiv(B, 64)), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<MStreamHeader*>(s), hd,
                       reinterpret_cast<long long*>(s + Ls.pos), reinterpret_cast<int*>(s + Ls.fresh), reset_mask_dev, B);
    HIPCHK(h, hipGetLastError());
    mine[state_dev] = B;
    (dec ? h->mimi_streams : h->mimi_dstreams).erase(state_dev);      // (the header just written ends its life as the other kind)
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
    return mstream_reset(h, state_dev, state_bytes, B, reset_mask_dev, stream, false);
}

int ac_mimi_stream_encode(ac_handle* h, void* state_dev, size_t state_bytes, const float* sig_dev, int B, int F, int K, int64_t* toks_dev,
                          void* ws, size_t ws_bytes, void* stream) {
    return mstream_encode(h, state_dev, state_bytes, B, nullptr, nullptr, B, sig_dev, F, K, toks_dev, ws, ws_bytes, stream, "ac_mimi_stream_encode");
}

int ac_mimi_stream_encode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                                const float* sig_dev, int F, int K, int64_t* toks_dev, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "ac_mimi_stream_encode_slots";
    const int rc = stream_slots_args(h, slots_host, slots_dev, who);
    return rc ? rc : mstream_encode(h, state_dev, state_bytes, B, slots_host, slots_dev, n, sig_dev, F, K, toks_dev, ws, ws_bytes, stream, who);
}

size_t ac_mimi_stream_decode_state_bytes(const ac_handle* h, int B) {
    if (!h || B < 1 || h->arch != ARCH_MIMI) return 0;
    return mdstream_layout(h, B).total;
}

size_t ac_mimi_stream_decode_workspace_bytes(const ac_handle* h, int B, int F) {
    if (!h || B < 1 || F < 1 || h->arch != ARCH_MIMI) return 0;
    return mdstream_plan_ws(h, B, F).total_bytes;
}

int ac_mimi_stream_decode_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream) {
    return mstream_reset(h, state_dev, state_bytes, B, reset_mask_dev, stream, true);
}

int ac_mimi_stream_decode(ac_handle* h, void* state_dev, size_t state_bytes, const int64_t* toks_dev, int B, int F, int K, float* sig_dev,
                          void* ws, size_t ws_bytes, void* stream) {
    return mstream_decode(h, state_dev, state_bytes, B, nullptr, nullptr, B, toks_dev, F, K, sig_dev, ws, ws_bytes, stream, "ac_mimi_stream_decode");
}

int ac_mimi_stream_decode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                                const int64_t* toks_dev, int F, int K, float* sig_dev, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "ac_mimi_stream_decode_slots";
    const int rc = stream_slots_args(h, slots_host, slots_dev, who);
    return rc ? rc : mstream_decode(h, state_dev, state_bytes, B, slots_host, slots_dev, n, toks_dev, F, K, sig_dev, ws, ws_bytes, stream, who);
}

}  // extern "C"
