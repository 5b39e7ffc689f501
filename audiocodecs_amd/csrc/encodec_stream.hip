// Streaming EnCodec encode and decode (include/audiocodecs_amd.h ac_encodec_stream_*; DESIGN.md "Streaming EnCodec").
// A push of F whole frames per stream runs the batch path's layers on [history | chunk]: every causal conv reads its last k - stride
// input rows from the stream state (stream_launch.h stream_stage, then the tap-GEMM with no left padding), every transposed conv its
// previous input row, and the LSTM starts from the h and c the previous push left (encodec_stream.h estream_lstm_step_kernel).
// EnCodec pads by reflection: a FRESH stream's history is the mirror image of its own first rows (STAGE_REFLECT; the ELU'd inputs of
// the residual blocks are mirrored after the ELU, as the batch kernels do), which is why the first push after a reset must bring
// warmup_frames() = max(kernel_size, last_kernel_size) frames: with fewer, the frame-rate convs would fall under the reference's
// small-input reflect rule and no later push could reproduce the one-shot result.  The fused batch-only kernels (enc_front / enc_stream,
// dec_tail / dec_stream, rb_stream6, rb_stream128m, rb_fused6) assume the clip start at row 0: a push goes through the per-conv tap-GEMMs.
// Split16 activation scales are taken per stream over the push.  The caller owns the state and the workspace; no entry point here
// allocates or synchronises.
#include "core.h"
#include "stream_launch.h"
#include "encodec_stream.h"

namespace acimpl {

// byte layout of a state buffer for B streams (every section 256-B aligned): header, position, fresh flag, the conv histories in layer
// order, then h [layers][B][D] and c [layers][B][D] of the LSTM
struct EStreamLayout {
    size_t pos = 0, fresh = 0;                 // int64 [B] frames pushed, int32 [B]
    std::vector<size_t> conv;
    std::vector<int> conv_P, conv_C;           //   rows (k - stride; 1 for a transposed conv) and channels of each
    size_t lstm_h = 0, lstm_c = 0, lstm_bytes = 0;   // lstm_bytes: h and c together (contiguous: one memset clears them)
    size_t total = 0;
    int B = 0;                                 // streams the state holds
};

static EStreamLayout estream_layout(const ac_handle* h, int B, bool dec) {
    const ac_config& c = h->cfg;
    EStreamLayout L;
    L.B = B;
    size_t off = align_up(sizeof(MStreamHeader), 256);
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
    L.pos = take((size_t)B * 8);
    L.fresh = take((size_t)B * 4);
    auto conv = [&](int P, int C) { L.conv.push_back(take((size_t)B * std::max(P, 1) * C * 4)); L.conv_P.push_back(P); L.conv_C.push_back(C); };
    const LstmPlan& lp = dec ? h->dec_lstm : h->enc_lstm;
    if (!dec) {   // encoder order: stem, (block k3, down-sampler) per ratio, final conv
        conv(c.kernel_size - 1, 1);
        int ch = c.num_filters;
        for (int i = 0; i < c.num_ratios; ++i) {
            conv(c.residual_kernel_size - 1, ch);
            conv(c.upsampling_ratios[c.num_ratios - 1 - i], ch);
            ch *= 2;
        }
        conv(c.last_kernel_size - 1, ch);
    } else {      // decoder order: first conv, (transposed conv input, block k3) per ratio, head conv
        conv(c.kernel_size - 1, c.hidden_size);
        int ch = h->D;
        for (int i = 0; i < c.num_ratios; ++i) {
            conv(1, ch);
            ch /= 2;
            conv(c.residual_kernel_size - 1, ch);
        }
        conv(c.last_kernel_size - 1, ch);
    }
    const size_t one = align_up((size_t)std::max(lp.layers, 1) * B * h->D * 4, 256);
    L.lstm_h = off;
    L.lstm_c = off + one;
    L.lstm_bytes = 2 * one;
    off += 2 * one;
    L.total = off;
    return L;
}

static unsigned long long estream_fingerprint(const ac_config& c) {
    ac_config k = c;
    k.device = 0;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&k);
    unsigned long long f = 1469598103934665603ULL;
    for (size_t i = 0; i < sizeof k; ++i) f = (f ^ b[i]) * 1099511628211ULL;
    return f;
}

// frames the first push after a reset must bring: the widest frame-rate conv (see the head of this file)
static int warmup_frames(const ac_handle* h) { return std::max(h->cfg.kernel_size, h->cfg.last_kernel_size); }

// (`slot`, here and below: the slot map of a push that runs B listed streams of the state's Ls.B -- stream_stage.h; null = all, in order)
static int estream_stage(ac_handle* h, hipStream_t st, char* state, const EStreamLayout& Ls, const int* slot, int l, const Act& x, int B, float* staged, size_t cap, int mode) {
    return stream_stage(h, st, reinterpret_cast<float*>(state + Ls.conv[l]), reinterpret_cast<const int*>(state + Ls.fresh), Ls.conv_P[l], Ls.conv_C[l], l, x, B,
                        staged, cap, mode, true, slot, Ls.B);
}

// Pushes of up to this many frames take the input projections of the LSTM through mstream_linear_kernel, longer ones through the
// tap-GEMM.  A function of F alone -- never of B -- so that a stream's arithmetic does not depend on how many share its launch.
// B F = 256 rows is where the two routes met on the Mimi decode stream (mimi_stream.hip MSTREAM_SKINNY_AUTO_ROWS): F = 4 at B = 64.
constexpr int ESTREAM_SKINNY_FRAMES = 4;

// gin[b][t][4D] = W_ih x[b][t] for the whole push (the bias joins in the step kernel); x is [B][F][D], rows contiguous
static int estream_lstm_proj(ac_handle* h, hipStream_t st, const PackedGemm& g, const Act& x, int B, int F, float* gin) {
    const int D = x.C;
    if (F <= ESTREAM_SKINNY_FRAMES && x.ts == D && x.bs == (long long)F * D && aligned16(x.p) && D % 4 == 0 && g.w_off % 4 == 0) {
        MStreamLinearParams p{};
        p.x = x.p;
        p.w = h->blob + g.w_off;
        p.y = gin;
        p.x_pitch = D;
        p.y_pitch = 4 * D;
        p.R = B * F;
        p.N = 4 * D;
        p.K = D;
        const dim3 grid((unsigned)p.N, (unsigned)cdiv(p.R, 8));
        ProfScope ps(h, st, "mstream_linear_kernel", 2.0 * p.R * p.N * (double)D, 4.0 * ((double)p.N * D + (double)p.R * (D + p.N)));
        if (mstream_linear_ks(D) == 4) hipLaunchKernelGGL((mstream_linear_kernel<8, 4>), grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL((mstream_linear_kernel<8, 1>), grid, dim3(64), 0, st, p);
        HIPCHK(h, hipGetLastError());
        return AC_OK;
    }
    Epi e;
    e.no_bias = true;
    return tap_layer(h, st, g, {make_seg(x, 1, 1, PAD_ZERO, 0, 0, nullptr)}, B, F, TapDst{Out{gin, nullptr}, (long long)F * 4 * D, 4LL * D}, e);
}

// x [B][F][D] -> ELU(lstm(x) + x) [B][F][D] at `yelu`, from the state's h / c, which it leaves at the push's last step
static int estream_lstm(ac_handle* h, hipStream_t st, const LstmPlan& lp, const Act& x, char* state, const EStreamLayout& Ls, const int* slot, const LstmWs& ws,
                        float* yelu, int B, int F, Act2* y) {
    const int D = lp.D, L = lp.layers;
    if (D % 64 != 0 || D > 512) return fail(h, AC_EINVAL, "LSTM width %d unsupported (need 64, 128, 256 or 512)", D);
    if (L < 1 || L > 2) return fail(h, AC_EINVAL, "%d LSTM layers unsupported (1 or 2)", L);
    float* hstate = reinterpret_cast<float*>(state + Ls.lstm_h);
    float* cstate = reinterpret_cast<float*>(state + Ls.lstm_c);
    // step 0 reads the carried h from a copy: the last step of a one-frame push rewrites the state's h while other workgroups still read it
    // (a slot push gathers its streams' rows into the same dense [L][B][D] copy)
    float* h_in = ws.c;
    if (!slot) {
        HIPCHK(h, hipMemcpyAsync(h_in, hstate, (size_t)L * B * D * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
        ProfScope ps(h, st, "estream_gather_h_kernel", 0.0, 8.0 * L * B * D);
        hipLaunchKernelGGL(estream_gather_h_kernel<>, dim3(grid_for((long long)L * B * (D / 4))), dim3(256), 0, st, hstate, h_in, slot, B, Ls.B, L, D);
        HIPCHK(h, hipGetLastError());
    }
    const long long FD = (long long)F * D;
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        float* gin = l == 0 ? ws.gin : ws.gin1;
        float* hseq = l == 0 ? ws.hseq0 : ws.hseq1;
        const Act in = l == 0 ? x : Act{ws.hseq0, FD, D, F, D};
        int rc = estream_lstm_proj(h, st, lp.ih[l], in, B, F, gin);
        if (rc) return rc;
        ProfScope ps(h, st, "estream_lstm_step_kernel", 2.0 * F * (double)B * 4 * D * D, (double)F * (4.0 * D * D * 4 + (double)B * D * 4 * 8), F);
        for (int t = 0; t < F; ++t) {
            EStreamLstmParams q{};
            q.wpk = h->blob + lp.hh_off[l];
            q.bias = h->blob + lp.ih[l].b_off;
            q.gin = gin + (long long)t * 4 * D;
            q.gin_bs = 4LL * FD;
            q.hprev = t == 0 ? h_in + (long long)l * B * D : hseq + (long long)(t - 1) * D;
            q.hprev_bs = t == 0 ? D : FD;
            q.hout = hseq + (long long)t * D;
            q.hout_bs = FD;
            q.hstate = t == F - 1 ? hstate + (long long)l * Ls.B * D : nullptr;
            q.c = cstate + (long long)l * Ls.B * D;
            q.slot = slot;
            q.cap = Ls.B;
            if (last) {
                q.skip = x.p + (long long)t * x.ts;
                q.skip_bs = x.bs;
                q.yelu = yelu + (long long)t * D;
                q.y_bs = FD;
            }
            q.B = B;
            q.D = D;
            const dim3 grid(D / 4, cdiv(B, 64)), block(256);
            switch (D / 64) {
                case 1: hipLaunchKernelGGL(estream_lstm_step_kernel<1>, grid, block, 0, st, q); break;
                case 2: hipLaunchKernelGGL(estream_lstm_step_kernel<2>, grid, block, 0, st, q); break;
                case 4: hipLaunchKernelGGL(estream_lstm_step_kernel<4>, grid, block, 0, st, q); break;
                case 8: hipLaunchKernelGGL(estream_lstm_step_kernel<8>, grid, block, 0, st, q); break;
                default: return fail(h, AC_EINVAL, "LSTM width %d unsupported by the stream's step kernel", D);
            }
        }
        HIPCHK(h, hipGetLastError());
    }
    const unsigned* am = amax_plus(h, st, x, 1.0f, B);   // |lstm(x) + x| <= 1 + amax(x)
    *y = act_pair(Out{nullptr, yelu}, FD, D, F, D, am, B);
    return AC_OK;
}

// residual block on [history | ELU(x)]: y = [ELU(conv_k3(ELU(x))) | x] [W1; Ws] + (b1 + bs), ELU'd (every consumer starts with ELU)
static int estream_resblock(ac_handle* h, hipStream_t st, char* state, const EStreamLayout& Ls, const int* slot, int l, const ResBlockPlan& rb, const Act2& x, int B,
                            WsPtrs& ws, size_t cap, Act2* y) {
    const int L = x.raw.L, ch = rb.C;
    float* stg = ws.take();
    int rc = estream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, STAGE_REFLECT);
    if (rc) return rc;
    float* hb = ws.take();
    Act2 hv;
    if ((rc = mstream_conv(h, st, rb.c3, staged_act(stg, B, L + Ls.conv_P[l], ch), h->cfg.residual_kernel_size, 1, L, Out{nullptr, hb}, B, &hv))) return rc;
    ws.give(stg);
    float* ye = ws.take();
    if ((rc = tap_layer(h, st, rb.fused, {make_seg(hv.elu, 1, 1, PAD_ZERO, 0, 0, nullptr), make_seg(x.raw, 1, 1, PAD_ZERO, 0, hv.elu.C, nullptr)}, B, L,
                        TapDst{Out{nullptr, ye}, (long long)L * ch, ch}, Epi{}, y)))
        return rc;
    ws.give(hb);
    return AC_OK;
}

static void estream_advance(hipStream_t st, char* state, const EStreamLayout& Ls, const int* slot, int B, int F) {
    hipLaunchKernelGGL(mstream_advance_kernel<>, dim3(cdiv(B, 64)), dim3(64), 0, st, reinterpret_cast<long long*>(state + Ls.pos),
                       reinterpret_cast<int*>(state + Ls.fresh), B, F, slot, Ls.B);
}

// one push: sig [B][F*hop] -> feats [B][F][H]; the stream state advances by F frames (encoder_fwd on [history | chunk])
static int estream_encoder(ac_handle* h, hipStream_t st, char* state, const EStreamLayout& Ls, const int* slot, const float* sig, int B, int F, float* feats,
                           WsPtrs& ws, size_t cap) {
    const ac_config& c = h->cfg;
    const int T = F * h->hop;
    int l = 0, rc;
    Act2 x, y;
    float* stg = ws.take();
    if ((rc = estream_stage(h, st, state, Ls, slot, l, Act{sig, (long long)T, 1, T, 1}, B, stg, cap, STAGE_REFLECT))) return rc;
    if ((rc = mstream_conv(h, st, h->enc_stem, staged_act(stg, B, T + Ls.conv_P[l], 1), c.kernel_size, 1, T, Out{ws.take(), ws.take()}, B, &x))) return rc;
    ws.give(stg);
    ++l;
    for (int i = 0; i < c.num_ratios; ++i) {
        const int ratio = c.upsampling_ratios[c.num_ratios - 1 - i];
        if ((rc = estream_resblock(h, st, state, Ls, slot, l, h->enc_rb[i], x, B, ws, cap, &y))) return rc;
        ws.give(x);
        x = y;
        ++l;
        // down-sampler (k = 2 * ratio, stride ratio) on [history | ELU(x)]
        const int L = x.elu.L, ch = x.elu.C;
        stg = ws.take();
        if ((rc = estream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, STAGE_REFLECT))) return rc;
        ws.give(x);
        const bool last = i == c.num_ratios - 1;     // the last one feeds the LSTM: raw only
        if ((rc = mstream_conv(h, st, h->enc_down[i], staged_act(stg, B, L + Ls.conv_P[l], ch), 2 * ratio, ratio, L / ratio,
                               Out{ws.take(), last ? nullptr : ws.take()}, B, &x)))
            return rc;
        ws.give(stg);
        ++l;
    }
    float* ye = ws.take();
    if ((rc = estream_lstm(h, st, h->enc_lstm, x.raw, state, Ls, slot, ws.lstm, ye, B, F, &y))) return rc;
    ws.give(x);
    x = y;
    stg = ws.take();
    if ((rc = estream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, STAGE_REFLECT))) return rc;
    ws.give(x);
    if ((rc = mstream_conv(h, st, h->enc_final, staged_act(stg, B, F + Ls.conv_P[l], h->D), c.last_kernel_size, 1, F, Out{feats, nullptr}, B, nullptr))) return rc;
    ws.give(stg);
    capture(h, st, Act{feats, (long long)F * c.hidden_size, c.hidden_size, F, c.hidden_size}, B);   // test hook: the push's features
    estream_advance(st, state, Ls, slot, B, F);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

// one push: toks [B][F][K] -> sig [B][F*hop]; the decode state advances by F frames (decoder_fwd on [history | chunk])
static int estream_decoder(ac_handle* h, hipStream_t st, char* state, const EStreamLayout& Ls, const int* slot, const long long* toks, int B, int F, int K, float* sig,
                           WsPtrs& ws, size_t cap) {
    const ac_config& c = h->cfg;
    const int H = c.hidden_size;
    int l = 0, rc;
    float* zb = ws.take();
    if ((rc = rvq_decode_fwd(h, st, toks, B * F, K, zb))) return rc;
    Act2 x, y;
    float* stg = ws.take();
    if ((rc = estream_stage(h, st, state, Ls, slot, l, Act{zb, (long long)F * H, H, F, H}, B, stg, cap, STAGE_REFLECT))) return rc;
    ws.give(zb);
    if ((rc = mstream_conv(h, st, h->dec_first, staged_act(stg, B, F + Ls.conv_P[l], H), c.kernel_size, 1, F, Out{ws.take(), nullptr}, B, &x))) return rc;
    ws.give(stg);
    ++l;
    float* ye = ws.take();
    if ((rc = estream_lstm(h, st, h->dec_lstm, x.raw, state, Ls, slot, ws.lstm, ye, B, F, &y))) return rc;
    ws.give(x);
    x = y;
    for (int i = 0; i < c.num_ratios; ++i) {
        const int ratio = c.upsampling_ratios[i], cin = h->dec_up[i].Ktot / 2, cup = h->dec_up[i].N / ratio, L = x.elu.L;
        // transposed conv (k = 2 ratio): output row m = [x[m-1] | x[m]] Wp (convtr_fwd), x[-1] from the cache (zeros when fresh)
        stg = ws.take();
        if ((rc = estream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, STAGE_ZERO))) return rc;
        ws.give(x);
        if ((rc = mstream_conv(h, st, h->dec_up[i], staged_act(stg, B, L + Ls.conv_P[l], cin), 2, 1, L, Out{ws.take(), ws.take()}, B, &y))) return rc;
        ws.give(stg);
        ++l;
        const int Lu = L * ratio;                      // [B][L][ratio * cup] is [B][L * ratio][cup]
        x.raw = Act{y.raw.p, (long long)Lu * cup, cup, Lu, cup, y.raw.amax, y.raw.amax_n};
        x.elu = Act{y.elu.p, (long long)Lu * cup, cup, Lu, cup, y.elu.amax, y.elu.amax_n};
        if ((rc = estream_resblock(h, st, state, Ls, slot, l, h->dec_rb[i], x, B, ws, cap, &y))) return rc;
        ws.give(x);
        x = y;
        ++l;
    }
    const int Ts = x.elu.L, Fh = x.elu.C;
    stg = ws.take();
    if ((rc = estream_stage(h, st, state, Ls, slot, l, x.elu, B, stg, cap, STAGE_REFLECT))) return rc;
    ws.give(x);
    if ((rc = mstream_conv(h, st, h->dec_head, staged_act(stg, B, Ts + Ls.conv_P[l], Fh), c.last_kernel_size, 1, Ts, Out{sig, nullptr}, B, nullptr))) return rc;
    ws.give(stg);
    estream_advance(st, state, Ls, slot, B, F);
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

// the batch plan for one frame more than the push: at every level a frame's rows outnumber the level's history, or the level is
// far narrower than the widest one (the frame-rate convs: k - 1 rows of D channels against a frame of hop * num_filters samples)
static Workspace estream_plan_ws(const ac_handle* h, int B, int F, bool dec) {
    return dec ? plan_ws(h, B, 0, F + 1, false) : plan_ws(h, B, (F + 1) * h->hop, 0, true);
}

static int estream_check(ac_handle* h, int B, bool dec, const char* who) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->arch != ARCH_ENCODEC) return fail(h, AC_EINVAL, "%s: not an EnCodec handle", who);
    if (!dec && !h->has_enc) return fail(h, AC_ESTATE, "%s: the handle was loaded without encoder weights (mode=\"decode\")", who);
    if (dec && !h->has_dec) return fail(h, AC_ESTATE, "%s: the handle was loaded without decoder weights (mode=\"encode\")", who);
    if (B < 1) return fail(h, AC_EINVAL, "%s: B=%d", who, B);
    return AC_OK;
}

static int estream_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream, bool dec) {
    const char* who = dec ? "ac_encodec_stream_decode_reset" : "ac_encodec_stream_reset";
    int rc = estream_check(h, B, dec, who);
    if (rc) return rc;
    if (!state_dev) return fail(h, AC_EINVAL, "%s: state is null", who);
    // (a lockstep stream's frame count is one per state; slots restart alone through ac_encodec_stream_reset_slots)
    if (reset_mask_dev) return fail(h, AC_EINVAL, "%s: EnCodec streams reset together (reset_mask_dev must be NULL)", who);
    const EStreamLayout Ls = estream_layout(h, B, dec);
    if (state_bytes < Ls.total) return fail(h, AC_ENOMEM, "%s: state of %zu bytes, %zu needed", who, state_bytes, Ls.total);
    if ((reinterpret_cast<uintptr_t>(state_dev) & 255) != 0) return fail(h, AC_EINVAL, "%s: state must be 256-byte aligned", who);
    char* s = static_cast<char*>(state_dev);
    hipStream_t st = (hipStream_t)stream;
    MStreamHeader hd{dec ? EDSTREAM_MAGIC : ESTREAM_MAGIC, 1u, estream_fingerprint(h->cfg), B, 0};
    hipLaunchKernelGGL(mstream_reset_kernel<>, dim3(cdiv(B, 64)), dim3(64), 0, st, reinterpret_cast<MStreamHeader*>(s), hd,
                       reinterpret_cast<long long*>(s + Ls.pos), reinterpret_cast<int*>(s + Ls.fresh), static_cast<const uint8_t*>(nullptr), B);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemsetAsync(s + Ls.lstm_h, 0, Ls.lstm_bytes, st));      // h = c = 0; the conv histories are rebuilt from the first push
    (dec ? h->encodec_dstreams : h->encodec_streams)[state_dev] = ac_handle::EStreamReg{B, std::vector<uint8_t>((size_t)B, 1)};
    (dec ? h->encodec_streams : h->encodec_dstreams).erase(state_dev);   // (the header just written ends its life as the other kind)
    return AC_OK;
}

// the handle's record of a state of `B` streams, and its layout, or the refusal
static int estream_find(ac_handle* h, void* state_dev, size_t state_bytes, int B, bool dec, const char* who, EStreamLayout* Ls,
                        ac_handle::EStreamReg** reg) {
    auto& mine = dec ? h->encodec_dstreams : h->encodec_streams;
    auto& other = dec ? h->encodec_streams : h->encodec_dstreams;
    auto it = mine.find(state_dev);
    if (it == mine.end())
        return fail(h, AC_EINVAL, "%s: the state was never reset as %s state on this handle%s", who, dec ? "a decode" : "an encode",
                    other.count(state_dev) ? (dec ? " (it is an encode state)" : " (it is a decode state)") : "");
    if (it->second.B != B) return fail(h, AC_EINVAL, "%s: the state holds %d streams, B=%d", who, it->second.B, B);
    *Ls = estream_layout(h, B, dec);
    if (state_bytes < Ls->total) return fail(h, AC_ENOMEM, "%s: state of %zu bytes, %zu needed", who, state_bytes, Ls->total);
    *reg = &it->second;
    return AC_OK;
}

// The checks of a push that touch nothing; *reg: the handle's record of the state.  `slots` (host; null: a lockstep push of all B
// streams): the n listed streams -- in range, distinct -- are the ones whose freshness decides the warm-up rule.
static int estream_push_check(ac_handle* h, void* state_dev, size_t state_bytes, const void* in, const void* out, int B, const int* slots, int n,
                              int F, int K, bool dec, const char* who, EStreamLayout* Ls, ac_handle::EStreamReg** reg) {
    int rc = estream_check(h, B, dec, who);
    if (rc) return rc;
    if (!state_dev || !in || !out || F < 1) return fail(h, AC_EINVAL, "%s: bad argument (F=%d)", who, F);
    if (K < 1 || K > h->cfg.num_quantizers) return fail(h, AC_EINVAL, "%s: K=%d outside [1, %d]", who, K, h->cfg.num_quantizers);
    if ((rc = estream_find(h, state_dev, state_bytes, B, dec, who, Ls, reg))) return rc;
    const std::vector<uint8_t>& fresh = (*reg)->fresh;
    bool any_fresh = false;
    if (slots) {
        if ((rc = stream_slots_check(h, slots, n, B, who))) return rc;
        for (int i = 0; i < n; ++i) any_fresh = any_fresh || fresh[slots[i]];
    } else {
        for (int b = 0; b < B; ++b) any_fresh = any_fresh || fresh[b];
    }
    if (any_fresh && F < warmup_frames(h))
        return fail(h, AC_EINVAL, "%s: the first push of a stream after its reset must bring %d frames (reflect padding of the frame-rate convs), got F=%d",
                    who, warmup_frames(h), F);
    return check_len(h, (long long)F * h->hop);
}

// ac_encodec_stream_reset_slots / _decode_reset_slots: the listed streams start afresh, the others and the header stay as they are
static int estream_reset_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n, void* stream,
                               bool dec) {
    const char* who = dec ? "ac_encodec_stream_decode_reset_slots" : "ac_encodec_stream_reset_slots";
    int rc = estream_check(h, B, dec, who);
    if (rc) return rc;
    if (!state_dev || !slots_host || !slots_dev) return fail(h, AC_EINVAL, "%s: null argument", who);
    EStreamLayout Ls;
    ac_handle::EStreamReg* reg = nullptr;
    if ((rc = estream_find(h, state_dev, state_bytes, B, dec, who, &Ls, &reg))) return rc;
    if ((rc = stream_slots_check(h, slots_host, n, B, who))) return rc;
    const LstmPlan& lp = dec ? h->dec_lstm : h->enc_lstm;
    char* s = static_cast<char*>(state_dev);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(estream_reset_slots_kernel<>, dim3(n), dim3(256), 0, st, reinterpret_cast<long long*>(s + Ls.pos), reinterpret_cast<int*>(s + Ls.fresh),
                       reinterpret_cast<float*>(s + Ls.lstm_h), reinterpret_cast<float*>(s + Ls.lstm_c), slots_dev, n, B, std::max(lp.layers, 1), h->D);
    HIPCHK(h, hipGetLastError());
    for (int i = 0; i < n; ++i) reg->fresh[slots_host[i]] = 1;
    return AC_OK;
}

// One push of n streams of a state of B: all of them in order (a lockstep push: slots_host = slots_dev = null, n = B) or the listed
// ones.  Every buffer and launch shape is that of a dense push of n streams; `slots_dev` only redirects the addresses into the state.
static int estream_encode(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                          const float* sig_dev, int F, int K, int64_t* toks_dev, void* ws, size_t ws_bytes, void* stream, const char* who) {
    EStreamLayout Ls;
    ac_handle::EStreamReg* reg = nullptr;
    int rc = estream_push_check(h, state_dev, state_bytes, sig_dev, toks_dev, B, slots_host, n, F, K, false, who, &Ls, &reg);
    if (rc) return rc;
    const Workspace w = estream_plan_ws(h, n, F, false);
    WsPtrs p;
    if ((rc = carve(h, w, ws, ws_bytes, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = amax_begin(h, st, n))) return rc;
    float* feats = p.lstm.gin;        // free again once the LSTM is done (as ac_encode)
    rc = estream_encoder(h, st, static_cast<char*>(state_dev), Ls, slots_dev, sig_dev, n, F, feats, p, w.act_floats);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) reg->fresh[slots_host ? slots_host[i] : i] = 0;
    return rvq_encode_fwd(h, st, feats, n * F, K, reinterpret_cast<long long*>(toks_dev));
}

static int estream_decode(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                          const int64_t* toks_dev, int F, int K, float* sig_dev, void* ws, size_t ws_bytes, void* stream, const char* who) {
    EStreamLayout Ls;
    ac_handle::EStreamReg* reg = nullptr;
    int rc = estream_push_check(h, state_dev, state_bytes, toks_dev, sig_dev, B, slots_host, n, F, K, true, who, &Ls, &reg);
    if (rc) return rc;
    const Workspace w = estream_plan_ws(h, n, F, true);
    WsPtrs p;
    if ((rc = carve(h, w, ws, ws_bytes, &p))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = amax_begin(h, st, n))) return rc;
    rc = estream_decoder(h, st, static_cast<char*>(state_dev), Ls, slots_dev, reinterpret_cast<const long long*>(toks_dev), n, F, K, sig_dev, p, w.act_floats);
    if (!rc)
        for (int i = 0; i < n; ++i) reg->fresh[slots_host ? slots_host[i] : i] = 0;
    return rc;
}

}  // namespace acimpl

using namespace acimpl;

extern "C" {

size_t ac_encodec_stream_state_bytes(const ac_handle* h, int B) {
    if (!h || B < 1 || h->arch != ARCH_ENCODEC) return 0;
    return estream_layout(h, B, false).total;
}

size_t ac_encodec_stream_workspace_bytes(const ac_handle* h, int B, int F) {
    if (!h || B < 1 || F < 1 || h->arch != ARCH_ENCODEC) return 0;
    return estream_plan_ws(h, B, F, false).total_bytes;
}

int ac_encodec_stream_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream) {
    return estream_reset(h, state_dev, state_bytes, B, reset_mask_dev, stream, false);
}

int ac_encodec_stream_encode(ac_handle* h, void* state_dev, size_t state_bytes, const float* sig_dev, int B, int F, int K, int64_t* toks_dev,
                             void* ws, size_t ws_bytes, void* stream) {
    return estream_encode(h, state_dev, state_bytes, B, nullptr, nullptr, B, sig_dev, F, K, toks_dev, ws, ws_bytes, stream, "ac_encodec_stream_encode");
}

size_t ac_encodec_stream_decode_state_bytes(const ac_handle* h, int B) {
    if (!h || B < 1 || h->arch != ARCH_ENCODEC) return 0;
    return estream_layout(h, B, true).total;
}

size_t ac_encodec_stream_decode_workspace_bytes(const ac_handle* h, int B, int F) {
    if (!h || B < 1 || F < 1 || h->arch != ARCH_ENCODEC) return 0;
    return estream_plan_ws(h, B, F, true).total_bytes;
}

int ac_encodec_stream_decode_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream) {
    return estream_reset(h, state_dev, state_bytes, B, reset_mask_dev, stream, true);
}

int ac_encodec_stream_decode(ac_handle* h, void* state_dev, size_t state_bytes, const int64_t* toks_dev, int B, int F, int K, float* sig_dev,
                             void* ws, size_t ws_bytes, void* stream) {
    return estream_decode(h, state_dev, state_bytes, B, nullptr, nullptr, B, toks_dev, F, K, sig_dev, ws, ws_bytes, stream, "ac_encodec_stream_decode");
}

int ac_encodec_stream_reset_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                                  void* stream) {
    return estream_reset_slots(h, state_dev, state_bytes, B, slots_host, slots_dev, n, stream, false);
}

int ac_encodec_stream_decode_reset_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                                         void* stream) {
    return estream_reset_slots(h, state_dev, state_bytes, B, slots_host, slots_dev, n, stream, true);
}

int ac_encodec_stream_encode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                                   const float* sig_dev, int F, int K, int64_t* toks_dev, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "ac_encodec_stream_encode_slots";
    const int rc = stream_slots_args(h, slots_host, slots_dev, who);
    return rc ? rc : estream_encode(h, state_dev, state_bytes, B, slots_host, slots_dev, n, sig_dev, F, K, toks_dev, ws, ws_bytes, stream, who);
}

int ac_encodec_stream_decode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev, int n,
                                   const int64_t* toks_dev, int F, int K, float* sig_dev, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "ac_encodec_stream_decode_slots";
    const int rc = stream_slots_args(h, slots_host, slots_dev, who);
    return rc ? rc : estream_decode(h, state_dev, state_bytes, B, slots_host, slots_dev, n, toks_dev, F, K, sig_dev, ws, ws_bytes, stream, who);
}

}  // extern "C"
