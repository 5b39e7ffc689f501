// WavLM x-vector speaker encoder: model plan, weight packing and the launch sequence of one embedding call.
// One translation unit of the library (core.h has the map): owns the kernels of wavlm.h and the ac_spk_* entry points.
//
//   [HF] = transformers models/wavlm/modeling_wavlm.py, WavLMForXVector.forward (:1557-1637):
//   conv front end (:723-782) -> LayerNorm + projection (:93-105) -> rows >= Lf zeroed, grouped positional conv, LayerNorm (:399-407)
//   -> post-LN layers with gated relative-position bias (:108-336) -> weighted sum of the hidden states (:1591-1595) -> projector,
//   TDNN layers (:1469-1498) -> mean | std over the clip's rows (:1604-1618) -> feature_extractor.
// Data layout: channels-last fp32 [B][time][C]; the transformer and the head's linear layers work on the merged [B*T][C] row matrix.
// A clip's result depends on nothing but that clip: per-clip scales in the convs, per-row scales in the linear layers, per-workgroup
// scales in the attention and the positional conv -- so the batch may be walked in chunks of any size.
#include "core.h"
#include "wavlm.h"

namespace acimpl {

constexpr int SPK_MAX_T = 6000;                       // frames per clip (two minutes): the attention's bias table lives in LDS
constexpr size_t SPK_WS_CAP = (size_t)1 << 30;        // workspace cap that sizes a chunk of clips when max_chunk_clips is 0

static void spk_lengths(const ac_spk_config& c, long long L, long long* Ls) {
    long long n = L;
    for (int i = 0; i < c.num_conv_layers; ++i) {
        n = n < c.conv_kernel[i] ? 0 : (n - c.conv_kernel[i]) / c.conv_stride[i] + 1;
        Ls[i] = n;
    }
}

struct SpkWs {
    int Bc = 0, T = 0;
    long long T0 = 0, T1 = 0;
    int nch = 0;
    size_t lens = 0, part = 0, mr = 0, bufA = 0, bufB = 0, x = 0, qkv = 0, att = 0, hid = 0, acc = 0, gate = 0, t0 = 0, t1 = 0, pooled = 0;   // byte offsets behind the pool
    size_t pool = 0, total = 0;
};

static size_t spk_clip_bytes(const ac_handle* h, long long L, SpkWs* w) {
    const ac_spk_config& c = h->scfg;
    long long Ls[AC_MAX_RATIOS];
    spk_lengths(c, L, Ls);
    const long long T0 = Ls[0], T1 = Ls[1], T = Ls[c.num_conv_layers - 1];
    const int H = c.hidden_size, I = c.intermediate_size, C = c.conv_dim;
    int tw = c.tdnn_dim[0];
    for (int i = 0; i < c.num_tdnn_layers; ++i) tw = std::max(tw, c.tdnn_dim[i]);
    const int nch = (int)((T0 + SPK_STEM_FT - 1) / SPK_STEM_FT);
    size_t o = 0;
    auto take = [&](size_t* dst, size_t floats) { if (dst) *dst = o; o += align_up(floats * 4, 256); };
    take(w ? &w->lens : nullptr, 2);
    take(w ? &w->part : nullptr, (size_t)nch * C * 2);
    take(w ? &w->mr : nullptr, (size_t)C * 2);
    take(w ? &w->bufA : nullptr, (size_t)T0 * C);
    take(w ? &w->bufB : nullptr, (size_t)T1 * C);
    take(w ? &w->x : nullptr, (size_t)T * H);
    take(w ? &w->qkv : nullptr, (size_t)T * 3 * H);
    take(w ? &w->att : nullptr, (size_t)T * H);
    take(w ? &w->hid : nullptr, (size_t)T * I);
    take(w ? &w->acc : nullptr, (size_t)T * H);
    take(w ? &w->gate : nullptr, (size_t)T * c.num_attention_heads);
    take(w ? &w->t0 : nullptr, (size_t)T * tw);
    take(w ? &w->t1 : nullptr, (size_t)T * tw);
    take(w ? &w->pooled : nullptr, (size_t)2 * tw);
    if (w) { w->T0 = T0; w->T1 = T1; w->T = (int)T; w->nch = nch; }
    return o;
}

// the layout of a pass over Bc clips: every region is Bc times its per-clip size (each rounded to 256 bytes per clip)
static SpkWs spk_plan_ws(const ac_handle* h, int B, long long L) {
    SpkWs w;
    const size_t per = spk_clip_bytes(h, L, &w);
    int Bc = h->scfg.max_chunk_clips;
    if (Bc <= 0) Bc = (int)std::max<size_t>(1, SPK_WS_CAP / std::max<size_t>(per, 1));
    w.Bc = std::min(B, Bc);
    w.pool = align_up(pool_bytes(w.Bc, (size_t)w.Bc * w.T), 256);
    size_t* offs[] = {&w.lens, &w.part, &w.mr, &w.bufA, &w.bufB, &w.x, &w.qkv, &w.att, &w.hid, &w.acc, &w.gate, &w.t0, &w.t1, &w.pooled};
    for (size_t* o : offs) *o = w.pool + *o * (size_t)w.Bc;
    w.total = w.pool + per * (size_t)w.Bc + 512;
    return w;
}

// one conv / TDNN layer through the tap-GEMM: x viewed as rows of s time steps, J taps `dil` rows apart, no padding, M output rows
static int spk_conv(ac_handle* h, hipStream_t st, const PackedGemm& g, const Act& x, int s, int J, int dil, int M, float* y, int gelu, int B, Act* out) {
    TapSeg sg = make_seg(x, s, J, PAD_ZERO, 0, 0, nullptr, 0, 0);
    sg.dil = dil;
    Epi e;
    e.gelu = gelu;
    Act2 o;
    if (int rc = tap_layer(h, st, g, {sg}, B, M, TapDst{Out{y, nullptr}, (long long)M * g.N, g.N}, e, &o)) return rc;
    *out = o.raw;
    return AC_OK;
}

static unsigned grid1d(long long n, int per) { return (unsigned)std::max<long long>(1, std::min<long long>((n + per - 1) / per, 65535LL * 16)); }

// nb clips from sig (pitch L): embeddings to emb [nb][D]; the stage pointers arrive already advanced to the chunk's first clip
// (hidden: plus its layer pitch B_all * T * H)
static int spk_chunk_fwd(ac_handle* h, hipStream_t st, const float* sig, const int* valid, int nb, long long L, float* emb, const ac_spk_stages& sg,
                         long long hidden_pitch, char* base, const SpkWs& w) {
    const ac_spk_config& c = h->scfg;
    const SpkPlan& m = h->spk;
    const int C = c.conv_dim, H = c.hidden_size, I = c.intermediate_size, heads = c.num_attention_heads, T = w.T;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    int* lens = reinterpret_cast<int*>(base + w.lens);
    float *bufA = F(w.bufA), *bufB = F(w.bufB), *x = F(w.x), *qkv = F(w.qkv), *att = F(w.att), *hid = F(w.hid), *acc = F(w.acc), *gate = F(w.gate);
    const long long rows = (long long)nb * T;
    int rc;
    {
        ProfScope ps(h, st, "spk_lens_kernel", 0.0, 12.0 * nb);
        hipLaunchKernelGGL(spk_lens_kernel, dim3(cdiv(nb, 64)), dim3(64), 0, st, valid, nb, L, T, m.shrink, lens);
        HIPCHK(h, hipGetLastError());
    }
    // ---- conv 1: moments over time per (clip, channel), then normalise + GELU, the pre-norm values recomputed in each pass
    Act a;
    {
        SpkStemParams p{};
        p.sig = sig;
        p.w = h->blob + m.stem_w;
        p.gn_w = h->blob + m.gn_w;
        p.gn_b = h->blob + m.gn_b;
        p.part = F(w.part);
        p.mr = F(w.mr);
        p.y = bufA;
        p.amax = amax_new(h);
        p.L = L;
        p.T0 = (int)w.T0;
        p.C = C;
        p.nch = w.nch;
        p.eps = 1e-5f;                                   // nn.GroupNorm's default ([HF]:731)
        const double work = 2.0 * SPK_STEM_K * nb * (double)w.T0 * C;
        {
            ProfScope ps(h, st, "spk_stem_stats_kernel", 2.0 * work, 4.0 * nb * (double)L);
            hipLaunchKernelGGL(spk_stem_stats_kernel, dim3(w.nch, nb), dim3(256), 0, st, p);
            hipLaunchKernelGGL(spk_stem_norm_kernel, dim3(cdiv(C, 256), nb), dim3(256), 0, st, p);
        }
        ProfScope ps(h, st, "spk_stem_apply_kernel", work, 4.0 * nb * ((double)L + (double)w.T0 * C));
        hipLaunchKernelGGL(spk_stem_apply_kernel, dim3(w.nch, nb), dim3(256), 0, st, p);
        HIPCHK(h, hipGetLastError());
        a = Act{bufA, w.T0 * C, C, (int)w.T0, C, p.amax, p.amax ? nb : 0};
    }
    // ---- convs 2..7 (no bias) + GELU, ping-pong between the two wide buffers
    long long Ls[AC_MAX_RATIOS];
    spk_lengths(c, L, Ls);
    for (int i = 1; i < c.num_conv_layers; ++i) {
        float* dst = a.p == bufA ? bufB : bufA;
        if ((rc = spk_conv(h, st, m.conv[i - 1], a, 2, c.conv_kernel[i] == 3 ? 2 : 1, 1, (int)Ls[i], dst, 1, nb, &a))) return rc;
    }
    if (sg.feat) HIPCHK(h, hipMemcpyAsync(sg.feat, a.p, (size_t)rows * C * 4, hipMemcpyDeviceToDevice, st));
    // ---- feature projection: LayerNorm(C) in place, Linear(C -> H); rows t >= Lf to zero
    const unsigned* ln_rows = nullptr;
    float* feat = const_cast<float*>(a.p);
    if ((rc = layernorm_fwd(h, st, feat, m.fp_ln_w, m.fp_ln_b, feat, rows, C, c.layer_norm_eps, &ln_rows))) return rc;
    {
        Epi e;
        e.rowmax_in = ln_rows;
        if ((rc = linear_rows(h, st, m.fp, feat, rows, C, C, 0, x, H, e))) return rc;
    }
    if (valid) {
        ProfScope ps(h, st, "spk_mask_rows_kernel", 0.0, 4.0 * rows * H);
        hipLaunchKernelGGL(spk_mask_rows_kernel, dim3(grid1d((long long)T * H / 4, 256 * 4), nb), dim3(256), 0, st, x, lens, T, H / 4);
        HIPCHK(h, hipGetLastError());
    }
    // ---- positional conv + bias + GELU + residual -> att, LayerNorm -> x
    {
        SpkPosConvParams p{x, reinterpret_cast<const _Float16*>(h->blob + m.pos_img), h->blob + m.pos_inv, h->blob + m.pos_b, att, T, H};
        const int G = c.num_conv_pos_embedding_groups, K = c.num_conv_pos_embeddings, CG = H / G;
        ProfScope ps(h, st, "spk_posconv16_kernel", 2.0 * rows * H * (double)CG * K, 8.0 * rows * H + 4.0 * (double)H * CG * K);
        const dim3 grid(cdiv(T, 128), G, nb);
        if (CG == 48 && K == 128) hipLaunchKernelGGL((spk_posconv16_kernel<48, 128>), grid, dim3(256), (SpkPosCfg<48, 128>::lds_bytes), st, p);
        else if (CG == 32 && K == 16) hipLaunchKernelGGL((spk_posconv16_kernel<32, 16>), grid, dim3(256), (SpkPosCfg<32, 16>::lds_bytes), st, p);
        else return fail(h, AC_EINVAL, "positional conv of %d taps over %d channels per group has no kernel", K, CG);
        HIPCHK(h, hipGetLastError());
    }
    if ((rc = layernorm_fwd(h, st, att, m.enc_ln_w, m.enc_ln_b, x, rows, H, c.layer_norm_eps, nullptr))) return rc;
    // ---- transformer layers (post-LN); every hidden state goes into the weighted sum (and the stage buffer) as it appears
    const int nl = c.num_hidden_layers;
    auto state = [&](int i) -> int {
        {
            ProfScope ps(h, st, "spk_axpy_kernel", 2.0 * rows * H, (i ? 12.0 : 8.0) * rows * H);
            hipLaunchKernelGGL(spk_axpy_kernel, dim3(grid1d(rows * H / 4, 256 * 4)), dim3(256), 0, st, reinterpret_cast<const f32x4*>(x),
                               reinterpret_cast<f32x4*>(acc), m.lw[i], i == 0 ? 1 : 0, rows * H / 4);
            HIPCHK(h, hipGetLastError());
        }
        if (sg.hidden) HIPCHK(h, hipMemcpyAsync(sg.hidden + (long long)i * hidden_pitch, x, (size_t)rows * H * 4, hipMemcpyDeviceToDevice, st));
        return AC_OK;
    };
    for (int l = 0; l < nl; ++l) {
        const SpkTfLayer& Ly = m.tf[l];
        if ((rc = state(l))) return rc;
        {
            const long long n = rows * heads;
            ProfScope ps(h, st, "spk_gate_kernel", 16.0 * rows * H, 4.0 * rows * H);
            hipLaunchKernelGGL(spk_gate_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, h->blob + Ly.gate_w, h->blob + Ly.gate_b,
                               h->blob + Ly.gate_c, gate, nb, T, heads);
            HIPCHK(h, hipGetLastError());
        }
        if ((rc = linear_rows(h, st, Ly.qkv, x, rows, H, H, 0, qkv, 3 * H))) return rc;
        {
            WavlmAttnParams p{qkv, att, gate, h->blob + m.bias_tab, lens, nb, T, H, m.R, 0.125f};
            const size_t lds = WavlmAttnCfg::lds_bytes(T);
            if ((rc = ensure_lds(h, reinterpret_cast<const void*>(wavlm_attn16_kernel), lds))) return rc;
            ProfScope ps(h, st, "wavlm_attn16_kernel", 4.0 * nb * heads * (double)T * T * 64, 16.0 * rows * H);
            hipLaunchKernelGGL(wavlm_attn16_kernel, dim3(cdiv(T, 64), heads, nb), dim3(256), lds, st, p);
            HIPCHK(h, hipGetLastError());
        }
        Epi ea;
        ea.res = x;
        ea.res_rs = H;
        if ((rc = linear_rows(h, st, Ly.o, att, rows, H, H, 0, x, H, ea))) return rc;
        if ((rc = layernorm_fwd(h, st, x, Ly.ln1_w, Ly.ln1_b, x, rows, H, c.layer_norm_eps, &ln_rows))) return rc;
        Epi eg;
        eg.gelu = 1;
        eg.rowmax_in = ln_rows;
        const unsigned* hid_rows = nullptr;
        eg.rowmax_out = &hid_rows;
        if ((rc = linear_rows(h, st, Ly.fc1, x, rows, H, H, 0, hid, I, eg))) return rc;
        Epi em;
        em.rowmax_in = hid_rows;
        em.res = x;
        em.res_rs = H;
        if ((rc = linear_rows(h, st, Ly.fc2, hid, rows, I, I, 0, x, H, em))) return rc;
        if ((rc = layernorm_fwd(h, st, x, Ly.ln2_w, Ly.ln2_b, x, rows, H, c.layer_norm_eps, nullptr))) return rc;
    }
    if ((rc = state(nl))) return rc;
    // ---- x-vector head: projector, TDNN layers (dilated convs without padding + ReLU), statistic pooling, feature_extractor
    float* t0 = F(w.t0);
    float* t1 = F(w.t1);
    if ((rc = linear_rows(h, st, m.proj, acc, rows, H, H, 0, t0, m.proj.N))) return rc;
    Act ta{t0, (long long)T * m.proj.N, m.proj.N, T, m.proj.N};
    int M = T;
    for (int i = 0; i < c.num_tdnn_layers; ++i) {
        M -= (c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i];
        float* dst = ta.p == t0 ? t1 : t0;
        if ((rc = spk_conv(h, st, m.tdnn[i], ta, 1, c.tdnn_kernel[i], c.tdnn_dilation[i], M, dst, 0, nb, &ta))) return rc;
        const long long n4 = (long long)nb * M * ta.C / 4;
        ProfScope ps(h, st, "spk_relu_kernel", (double)n4 * 4, 32.0 * n4);
        hipLaunchKernelGGL(spk_relu_kernel, dim3(grid1d(n4, 256 * 4)), dim3(256), 0, st, reinterpret_cast<f32x4*>(dst), n4);
        HIPCHK(h, hipGetLastError());
    }
    const int last = ta.C;
    if (sg.tdnn) HIPCHK(h, hipMemcpyAsync(sg.tdnn, ta.p, (size_t)nb * M * last * 4, hipMemcpyDeviceToDevice, st));
    float* pooled = F(w.pooled);
    {
        ProfScope ps(h, st, "spk_pool_kernel", 5.0 * nb * (double)M * last, 8.0 * nb * (double)M * last);
        hipLaunchKernelGGL(spk_pool_kernel, dim3(cdiv(last, 256), nb), dim3(256), 0, st, ta.p, lens, M, last, pooled);
        HIPCHK(h, hipGetLastError());
    }
    if (sg.pooled) HIPCHK(h, hipMemcpyAsync(sg.pooled, pooled, (size_t)nb * 2 * last * 4, hipMemcpyDeviceToDevice, st));
    return linear_rows(h, st, m.fe, pooled, nb, 2 * last, 2 * last, 0, emb, m.fe.N);
}

// ---------------------------------------------------------------------------------------------
// weight packing (WavLMForXVector state-dict keys; checkpoint.synthetic_wavlm_sv_state_dict is the Python twin)
// ---------------------------------------------------------------------------------------------
int spk_finalize(ac_handle* h, Packer& pk) {
    const ac_spk_config& c = h->scfg;
    SpkPlan& m = h->spk;
    if (!pk.use16()) return fail(h, AC_EINVAL, "the speaker encoder runs in split16 arithmetic only (precision \"fp32\")");
    const int C = c.conv_dim, H = c.hidden_size, I = c.intermediate_size, heads = c.num_attention_heads;
    auto vec = [&](const std::string& name, size_t nel, size_t& off) {
        const std::vector<float>* v = pk.get(name, nel);
        if (!v) return false;
        off = pk.reserve(nel);
        std::copy(v->begin(), v->end(), pk.blob.begin() + off);
        return true;
    };
    // Linear layers; several names stack along the output axis (q | k | v)
    auto linear = [&](const std::vector<std::string>& names, int out_each, int in, PackedGemm& g) {
        g.N = out_each * (int)names.size();
        g.Ktot = in;
        g.has_bias = true;
        g.w_off = pk.reserve((size_t)g.N * in);
        for (size_t j = 0; j < names.size(); ++j) {
            const std::vector<float>* w = pk.get(names[j] + ".weight", (size_t)out_each * in);
            if (!w) return false;
            std::copy(w->begin(), w->end(), pk.blob.begin() + g.w_off + j * (size_t)out_each * in);
        }
        g.b_off = pk.reserve(g.N);
        for (size_t j = 0; j < names.size(); ++j) {
            const std::vector<float>* b = pk.get(names[j] + ".bias", (size_t)out_each);
            if (!b) return false;
            std::copy(b->begin(), b->end(), pk.blob.begin() + g.b_off + j * (size_t)out_each);
        }
        pk.pack6(g);
        return true;
    };
    const std::string fx = "wavlm.feature_extractor.conv_layers.";
    if (!vec(fx + "0.conv.weight", (size_t)C * SPK_STEM_K, m.stem_w) || !vec(fx + "0.layer_norm.weight", C, m.gn_w) || !vec(fx + "0.layer_norm.bias", C, m.gn_b))
        return pk.rc;
    m.conv.resize(c.num_conv_layers - 1);
    for (int i = 1; i < c.num_conv_layers; ++i) {
        // [C][C][k] -> [n][tap * C + ci]; a k3 / s2 conv reads two rows of two time steps: its fourth tap is zero
        const int k = c.conv_kernel[i], taps = k == 3 ? 4 : 2;
        const std::vector<float>* w = pk.get(fx + std::to_string(i) + ".conv.weight", (size_t)C * C * k);
        if (!w) return pk.rc;
        PackedGemm& g = m.conv[i - 1];
        g.N = C;
        g.Ktot = taps * C;
        g.has_bias = false;
        g.w_off = pk.reserve((size_t)g.N * g.Ktot);
        for (int n = 0; n < C; ++n)
            for (int ci = 0; ci < C; ++ci)
                for (int t = 0; t < k; ++t) pk.blob[g.w_off + (size_t)n * g.Ktot + (size_t)t * C + ci] = (*w)[((size_t)n * C + ci) * k + t];
        pk.pack6(g);
    }
    if (!vec("wavlm.feature_projection.layer_norm.weight", C, m.fp_ln_w) || !vec("wavlm.feature_projection.layer_norm.bias", C, m.fp_ln_b) ||
        !linear({"wavlm.feature_projection.projection"}, H, C, m.fp))
        return pk.rc;
    {   // positional conv [H][CG][K], weight norm over dims (0, 1) per tap ([HF]:77: dim = 2) folded here when (g, v) were given
        const int G = c.num_conv_pos_embedding_groups, K = c.num_conv_pos_embeddings, CG = H / G;
        const std::string pc = "wavlm.encoder.pos_conv_embed.conv";
        const size_t n = (size_t)H * CG * K;
        std::vector<float> w;
        auto it = h->host.find(pc + ".weight");
        if (it != h->host.end() && it->second.size() == n) {
            w = it->second;
        } else {
            const std::vector<float>* g0 = pk.get(pc + ".parametrizations.weight.original0", (size_t)K);
            const std::vector<float>* v = pk.get(pc + ".parametrizations.weight.original1", n);
            if (!g0 || !v) return pk.rc;
            w.resize(n);
            for (int j = 0; j < K; ++j) {
                double ss = 0.0;
                for (size_t r = 0; r < (size_t)H * CG; ++r) ss += (double)(*v)[r * K + j] * (*v)[r * K + j];
                const float scale = (*g0)[j] / (float)std::sqrt(ss);
                for (size_t r = 0; r < (size_t)H * CG; ++r) w[r * K + j] = (*v)[r * K + j] * scale;
            }
        }
        const size_t src = pk.reserve(n);
        for (int o = 0; o < H; ++o)
            for (int ci = 0; ci < CG; ++ci)
                for (int j = 0; j < K; ++j) pk.blob[src + (size_t)o * K * CG + (size_t)j * CG + ci] = w[((size_t)o * CG + ci) * K + j];
        std::vector<int> km((size_t)K * CG);
        for (size_t k = 0; k < km.size(); ++k) km[k] = (int)k;
        m.pos_img = pk.frag16(src, H, K * CG, km, &m.pos_inv);
        if (!vec(pc + ".bias", H, m.pos_b)) return pk.rc;
    }
    if (!vec("wavlm.encoder.layer_norm.weight", H, m.enc_ln_w) || !vec("wavlm.encoder.layer_norm.bias", H, m.enc_ln_b)) return pk.rc;
    m.tf.resize(c.num_hidden_layers);
    for (int l = 0; l < c.num_hidden_layers; ++l) {
        const std::string p = "wavlm.encoder.layers." + std::to_string(l);
        SpkTfLayer& Ly = m.tf[l];
        const bool ok = linear({p + ".attention.q_proj", p + ".attention.k_proj", p + ".attention.v_proj"}, H, H, Ly.qkv) &&
                        linear({p + ".attention.out_proj"}, H, H, Ly.o) && linear({p + ".feed_forward.intermediate_dense"}, I, H, Ly.fc1) &&
                        linear({p + ".feed_forward.output_dense"}, H, I, Ly.fc2) && vec(p + ".layer_norm.weight", H, Ly.ln1_w) &&
                        vec(p + ".layer_norm.bias", H, Ly.ln1_b) && vec(p + ".final_layer_norm.weight", H, Ly.ln2_w) &&
                        vec(p + ".final_layer_norm.bias", H, Ly.ln2_b) && vec(p + ".attention.gru_rel_pos_linear.weight", 8 * 64, Ly.gate_w) &&
                        vec(p + ".attention.gru_rel_pos_linear.bias", 8, Ly.gate_b) && vec(p + ".attention.gru_rel_pos_const", heads, Ly.gate_c);
        if (!ok) return pk.rc;
    }
    {   // E[bucket(delta)][h] for delta in [-R, R]: layer 0's embedding is shared by all layers ([HF]:384, 430)
        m.R = 2 * c.max_bucket_distance;
        const std::vector<float>* E = pk.get("wavlm.encoder.layers.0.attention.rel_attn_embed.weight", (size_t)c.num_buckets * heads);
        const std::vector<float>* tb = pk.get("spk.bucket_table", (size_t)2 * m.R + 1);
        if (!E || !tb) return pk.rc;
        m.bias_tab = pk.reserve((size_t)heads * (2 * m.R + 1));
        for (int i = 0; i <= 2 * m.R; ++i) {
            const float bf = (*tb)[i];
            const int bk = (int)bf;
            if (!(bf >= 0.f) || bk >= c.num_buckets || (float)bk != bf) return fail(h, AC_EINVAL, "spk.bucket_table[%d] = %g is no bucket index below %d", i, (double)bf, c.num_buckets);
            for (int hh = 0; hh < heads; ++hh) pk.blob[m.bias_tab + (size_t)hh * (2 * m.R + 1) + i] = (*E)[(size_t)bk * heads + hh];
        }
    }
    {   // softmax(layer_weights) in fp32, as torch evaluates it: exp(x - max) / sum
        const std::vector<float>* lw = pk.get("layer_weights", (size_t)c.num_hidden_layers + 1);
        if (!lw) return pk.rc;
        float mx = -INFINITY, sum = 0.f;
        for (float v : *lw) mx = std::max(mx, v);
        m.lw.resize(lw->size());
        for (size_t i = 0; i < lw->size(); ++i) { m.lw[i] = std::exp((*lw)[i] - mx); sum += m.lw[i]; }
        for (float& v : m.lw) v /= sum;
    }
    if (!linear({"projector"}, c.tdnn_dim[0], H, m.proj)) return pk.rc;
    m.tdnn.resize(c.num_tdnn_layers);
    m.shrink = 0;
    for (int i = 0; i < c.num_tdnn_layers; ++i) {
        // nn.Linear(in * k, out) viewed [out][k][in] ([HF]:1493): already the tap-GEMM's [n][tap * in + ci]
        const int in = c.tdnn_dim[i > 0 ? i - 1 : 0];
        if (!linear({"tdnn." + std::to_string(i) + ".kernel"}, c.tdnn_dim[i], in * c.tdnn_kernel[i], m.tdnn[i])) return pk.rc;
        m.shrink += (c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i];
    }
    if (!linear({"feature_extractor"}, c.xvector_output_dim, 2 * c.tdnn_dim[c.num_tdnn_layers - 1], m.fe)) return pk.rc;
    return AC_OK;
}

}  // namespace acimpl

extern "C" {

int ac_spk_create(const ac_spk_config* cfg, ac_handle** out) {
    if (!cfg || !out) return AC_EINVAL;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(ac_spk_config)) return AC_EINVAL;
    const ac_spk_config& c = *cfg;
    static const int kern[7] = {10, 3, 3, 3, 3, 2, 2}, strd[7] = {5, 2, 2, 2, 2, 2, 2};
    if (!c.feat_extract_norm_group || c.conv_bias || c.do_stable_layer_norm || !c.use_weighted_layer_sum || c.add_adapter) return AC_EINVAL;
    if (c.num_conv_layers != 7) return AC_EINVAL;
    for (int i = 0; i < 7; ++i)
        if (c.conv_kernel[i] != kern[i] || c.conv_stride[i] != strd[i]) return AC_EINVAL;
    if (c.conv_dim < 32 || c.conv_dim > 1024 || (c.conv_dim & (c.conv_dim - 1))) return AC_EINVAL;      // (the stem's thread layout: a power of two)
    if (c.num_attention_heads < 1 || c.hidden_size != 64 * c.num_attention_heads || c.hidden_size > 1024) return AC_EINVAL;   // head dim 64
    if (c.num_hidden_layers < 1 || c.num_hidden_layers > 64 || c.intermediate_size < 16 || c.intermediate_size % 4) return AC_EINVAL;
    const int G = c.num_conv_pos_embedding_groups, K = c.num_conv_pos_embeddings;
    if (G < 1 || c.hidden_size % G) return AC_EINVAL;
    if (!((c.hidden_size / G == 48 && K == 128) || (c.hidden_size / G == 32 && K == 16))) return AC_EINVAL;     // the two positional convs with a kernel
    if (c.num_buckets < 4 || c.num_buckets % 4 || c.max_bucket_distance <= c.num_buckets / 4 || c.max_bucket_distance > 4096) return AC_EINVAL;
    if (c.num_tdnn_layers < 1 || c.num_tdnn_layers > AC_MAX_RATIOS || c.xvector_output_dim < 1) return AC_EINVAL;
    int shrink = 0;
    for (int i = 0; i < c.num_tdnn_layers; ++i) {
        if (c.tdnn_dim[i] < 4 || c.tdnn_dim[i] % 4 || c.tdnn_kernel[i] < 1 || c.tdnn_kernel[i] > 8 || c.tdnn_dilation[i] < 1) return AC_EINVAL;
        if ((c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i] > 7) return AC_EINVAL;
        shrink += (c.tdnn_kernel[i] - 1) * c.tdnn_dilation[i];
    }
    if (shrink != 14) return AC_EINVAL;         // (the pooled-row rule min(Lf - 8, T - 14) is this stack's)
    if (!(c.layer_norm_eps > 0.f) || c.max_chunk_clips < 0) return AC_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c.device || c.device < 0) return AC_ENODEV;
    ac_handle* h = new (std::nothrow) ac_handle();
    if (!h) return AC_ENOMEM;
    h->arch = ARCH_SPK;
    h->scfg = c;
    h->hop = 320;
    h->D = c.xvector_output_dim;
    *out = h;
    return AC_OK;
}

int ac_spk_num_frames(long long L) { return L < 400 ? 0 : (int)std::min<long long>((L - 400) / 320 + 1, 0x7fffffff); }

size_t ac_spk_workspace_bytes(const ac_handle* h, int B, long long L) {
    if (!h || h->arch != ARCH_SPK || B < 1 || L < 400) return 0;
    return spk_plan_ws(h, B, L).total;
}

int ac_spk_embed(ac_handle* h, const float* sig_dev, const int32_t* valid_dev, int B, long long L, float* emb_out, const ac_spk_stages* stages,
                 void* ws, size_t ws_bytes, void* stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->arch != ARCH_SPK) return fail(h, AC_EINVAL, "ac_spk_embed: not a speaker-encoder handle (ac_spk_create)");
    if (!sig_dev || !emb_out || B < 1 || L < 1) return fail(h, AC_EINVAL, "ac_spk_embed: bad argument (B=%d, L=%lld)", B, L);
    const ac_spk_config& c = h->scfg;
    const int T = ac_spk_num_frames(L);
    if (T - h->spk.shrink < 1) return fail(h, AC_EINVAL, "ac_spk_embed: %lld samples give %d frames, the TDNN layers need %d: no row to pool (pad to 4880 samples)", L, T, h->spk.shrink + 1);
    if (T > SPK_MAX_T) return fail(h, AC_EINVAL, "ac_spk_embed: %d frames per clip exceed the limit of %d: split the clip", T, SPK_MAX_T);
    if (!ws) return fail(h, AC_EINVAL, "workspace pointer is null");
    const SpkWs w = spk_plan_ws(h, B, L);
    if (w.T != T) return fail(h, AC_EINVAL, "ac_spk_embed: the conv stack gives %d frames where the formula gives %d", w.T, T);
    if (ws_bytes < w.total) return fail(h, AC_ENOMEM, "workspace too small: %zu < %zu bytes", ws_bytes, w.total);
    char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    const int H = c.hidden_size, C = c.conv_dim, last = c.tdnn_dim[c.num_tdnn_layers - 1], M = T - h->spk.shrink;
    for (int b0 = 0; b0 < B; b0 += w.Bc) {
        const int nb = std::min(w.Bc, B - b0);
        pool_bind(h, base, w.Bc, (size_t)w.Bc * T);
        if ((rc = amax_begin(h, st, nb))) return rc;      // every chunk starts with fresh amax slots
        ac_spk_stages sg{};
        if (stages) {
            sg.feat = stages->feat ? stages->feat + (size_t)b0 * T * C : nullptr;
            sg.hidden = stages->hidden ? stages->hidden + (size_t)b0 * T * H : nullptr;
            sg.tdnn = stages->tdnn ? stages->tdnn + (size_t)b0 * M * last : nullptr;
            sg.pooled = stages->pooled ? stages->pooled + (size_t)b0 * 2 * last : nullptr;
        }
        rc = spk_chunk_fwd(h, st, sig_dev + (size_t)b0 * L, valid_dev ? reinterpret_cast<const int*>(valid_dev) + b0 : nullptr, nb, L,
                           emb_out + (size_t)b0 * c.xvector_output_dim, sg, (long long)B * T * H, base, w);
        if (rc) return rc;
    }
    return AC_OK;
}

int ac_spk_cosine(const float* a_dev, const float* b_dev, int B, int D, float* out_dev, void* stream) {
    if (!a_dev || !b_dev || !out_dev || B < 0 || D < 1) return AC_EINVAL;
    if (B == 0) return AC_OK;
    hipLaunchKernelGGL(spk_cosine_kernel, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, (hipStream_t)stream, a_dev, b_dev, B, D, out_dev);
    return hipGetLastError() == hipSuccess ? AC_OK : AC_EHIP;
}

}  // extern "C"
