// lm_path.hip: the Llama decoder with a KV cache (llama.h) -- plan, finalize, the state's layout, the launch
// sequences of a forward over T rows and of one generated token, and the ac_lm_* entry points.  Weights stay fp32 and every product is an
// fp32 FMA: at M <= 64 rows a layer is bound by the one pass over its weights, not by arithmetic.
#include "core.h"
#include "llama.h"

namespace acimpl {

namespace {

struct LmDims {
    int L, dim, ffn, nh, nkv, hd, nq, nkvd, C, ncb, pd, rows;
};

LmDims lm_dims(const ac_lm_config& c) {
    LmDims d;
    d.L = c.n_layers; d.dim = c.dim; d.ffn = c.ffn_dim; d.nh = c.n_heads; d.nkv = c.n_kv_heads; d.hd = c.dim / c.n_heads;
    d.nq = d.nh * d.hd; d.nkvd = d.nkv * d.hd; d.C = c.vocab_size; d.ncb = c.num_codebooks; d.pd = c.prompt_dim; d.rows = 2 * c.max_seq_len;
    return d;
}

struct LmState {
    int* hdr;
    int* alive;
    int* lens;
    long long* tok;
    float* pend;
    long long* hyp;
    float* kv;
    size_t plane;      // floats of one K (or V) plane: B * cap * nkv * hd
};

void lm_layout(const LmDims& d, int B, int cap, int max_steps, ac_lm_layout* o) {
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t r = at; at += align_up(bytes, 256); return r; };
    o->hdr = (long long)take(LM_HDR_WORDS * 4);
    o->alive = (long long)take(LM_MAX_ROWS * 4);
    o->lens = (long long)take(LM_MAX_ROWS * 4);
    o->tok = (long long)take(LM_MAX_ROWS * 8);
    o->logits = (long long)take((size_t)B * d.C * 4);
    o->hyp = (long long)take((size_t)B * std::max(max_steps, 1) * 8);
    const size_t plane = align_up((size_t)B * cap * d.nkvd * 4, 256);
    o->kv = (long long)take(2 * plane * d.L);
    o->plane_bytes = (long long)plane;
    o->total = (long long)at;
}

LmState lm_state(const LmDims& d, void* state, int B, int cap, int max_steps) {
    ac_lm_layout o;
    lm_layout(d, B, cap, max_steps, &o);
    char* base = static_cast<char*>(state);
    LmState s;
    s.hdr = reinterpret_cast<int*>(base + o.hdr);
    s.alive = reinterpret_cast<int*>(base + o.alive);
    s.lens = reinterpret_cast<int*>(base + o.lens);
    s.tok = reinterpret_cast<long long*>(base + o.tok);
    s.pend = reinterpret_cast<float*>(base + o.logits);
    s.hyp = reinterpret_cast<long long*>(base + o.hyp);
    s.kv = reinterpret_cast<float*>(base + o.kv);
    s.plane = (size_t)o.plane_bytes / 4;
    return s;
}

// workspace of a call over T rows per batch entry: x | q | att | hidden | the attention partials of one chunk of rows
struct LmWs {
    size_t x, q, att, hid, part, total;
    int Tc, S;         // rows per batch entry in one attention chunk; splits of the capacity
};

LmWs lm_plan_ws(const LmDims& d, int B, int T, int cap) {
    LmWs w;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t r = at; at += align_up(bytes, 256); return r; };
    const size_t M = (size_t)B * T;
    w.x = take(M * d.dim * 4);
    w.q = take(M * d.nq * 4);
    w.att = take(M * d.nq * 4);
    w.hid = take(M * d.ffn * 4);
    w.S = cdiv(cap, LM_KS);
    const size_t per_row = (size_t)d.nh * w.S * (d.hd + 2) * 4;            // one query row's partials
    long long tc = (long long)((64ull << 20) / (per_row * B));             // at most 64 MiB of partials ...
    tc = std::min<long long>(tc, 65535 / B);                               // ... and a grid's z extent
    w.Tc = (int)std::max<long long>(1, std::min<long long>(tc, T));
    w.part = take(per_row * B * w.Tc);
    w.total = at + 256;
    return w;
}

int rt_of(int M) { return M >= 8 ? 8 : M >= 4 ? 4 : M >= 2 ? 2 : 1; }

template <int EPI>
void launch_gemv(hipStream_t st, const LmGemv& p) {
    const int M = p.r.B * p.r.T, rt = rt_of(M);
    const dim3 grid((unsigned)cdiv(p.pairs, 4), (unsigned)std::min(cdiv(M, rt), 1024)), block(256);
    switch (rt) {
        case 8: hipLaunchKernelGGL((lm_gemv_kernel<EPI, 8>), grid, block, 0, st, p); break;
        case 4: hipLaunchKernelGGL((lm_gemv_kernel<EPI, 4>), grid, block, 0, st, p); break;
        case 2: hipLaunchKernelGGL((lm_gemv_kernel<EPI, 2>), grid, block, 0, st, p); break;
        default: hipLaunchKernelGGL((lm_gemv_kernel<EPI, 1>), grid, block, 0, st, p); break;
    }
}

template <int G>
void launch_attn_g(hipStream_t st, const LmAttn& p, const dim3& grid) {
    const int dpl = cdiv(p.hd, 64);
    if (dpl == 1) hipLaunchKernelGGL((lm_attn_kernel<G, 1>), grid, dim3(256), 0, st, p);
    else if (dpl == 2) hipLaunchKernelGGL((lm_attn_kernel<G, 2>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((lm_attn_kernel<G, 4>), grid, dim3(256), 0, st, p);
}

void launch_attn(hipStream_t st, const LmAttn& p) {
    const int M = p.r.B * p.r.T;
    const dim3 grid((unsigned)p.S, (unsigned)p.nkv, (unsigned)M);
    switch (p.nh / p.nkv) {
        case 1: launch_attn_g<1>(st, p, grid); break;
        case 2: launch_attn_g<2>(st, p, grid); break;
        case 4: launch_attn_g<4>(st, p, grid); break;
        default: launch_attn_g<8>(st, p, grid); break;
    }
    const dim3 cgrid((unsigned)p.nh, (unsigned)M);
    const int dpl = cdiv(p.hd, 64);
    if (dpl == 1) hipLaunchKernelGGL((lm_attn_combine_kernel<1>), cgrid, dim3(64), 0, st, p);
    else if (dpl == 2) hipLaunchKernelGGL((lm_attn_combine_kernel<2>), cgrid, dim3(64), 0, st, p);
    else hipLaunchKernelGGL((lm_attn_combine_kernel<4>), cgrid, dim3(64), 0, st, p);
}

// The layers over the rows (b, i), i < T, that sit in w.x, and the final norm's head(s).  `all_out` [B][T][C] or null; the last row's
// logits always go to the state's pending slot.
int lm_layers(ac_handle* h, hipStream_t st, const LmState& s, int B, int T, int cap, char* base, const LmWs& w, float* all_out, const ac_lm_stages* sg) {
    const ac_lm_config& c = h->lcfg;
    const LmDims d = lm_dims(c);
    const LmPlan& m = h->lm;
    float* x = reinterpret_cast<float*>(base + w.x);
    float* q = reinterpret_cast<float*>(base + w.q);
    float* att = reinterpret_cast<float*>(base + w.att);
    float* hid = reinterpret_cast<float*>(base + w.hid);
    float* part = reinterpret_cast<float*>(base + w.part);
    const LmRows all{B, T, 0, 1, T};
    const size_t M = (size_t)B * T;
    for (int l = 0; l < d.L; ++l) {
        const LmLayer& ly = m.layers[l];
        float* kc = s.kv + (size_t)(2 * l) * s.plane;
        float* vc = kc + s.plane;
        LmGemv g{};
        g.hdr = s.hdr; g.x = x; g.nw = h->blob + ly.an; g.wa = h->blob + ly.wqkv; g.K = d.dim; g.N = d.nq + 2 * d.nkvd; g.pairs = g.N / 2;
        g.eps = c.norm_eps; g.r = all; g.out = q; g.kc = kc; g.vc = vc; g.rcos = h->blob + m.rope_cos; g.rsin = h->blob + m.rope_sin;
        g.cap = cap; g.nq = d.nq; g.nkvd = d.nkvd; g.hd = d.hd;
        launch_gemv<LM_EPI_QKV>(st, g);
        for (int i0 = 0; i0 < T; i0 += w.Tc) {
            LmAttn a{};
            a.hdr = s.hdr; a.q = q; a.kc = kc; a.vc = vc; a.part = part; a.out = att;
            a.r = LmRows{B, std::min(w.Tc, T - i0), i0, 1, T};
            a.cap = cap; a.nh = d.nh; a.nkv = d.nkv; a.hd = d.hd; a.S = w.S; a.scale = 1.0f / std::sqrt((float)d.hd);
            launch_attn(st, a);
        }
        LmGemv o{};
        o.hdr = s.hdr; o.x = att; o.wa = h->blob + ly.wo; o.K = d.nq; o.N = d.dim; o.pairs = d.dim / 2; o.r = all; o.out = x;
        launch_gemv<LM_EPI_RES>(st, o);
        LmGemv f{};
        f.hdr = s.hdr; f.x = x; f.nw = h->blob + ly.fn; f.wa = h->blob + ly.w1; f.wb = h->blob + ly.w3; f.K = d.dim; f.N = d.ffn; f.pairs = d.ffn;
        f.eps = c.norm_eps; f.r = all; f.out = hid;
        launch_gemv<LM_EPI_SWIGLU>(st, f);
        LmGemv e{};
        e.hdr = s.hdr; e.x = hid; e.wa = h->blob + ly.w2; e.K = d.ffn; e.N = d.dim; e.pairs = d.dim / 2; e.r = all; e.out = x;
        launch_gemv<LM_EPI_RES>(st, e);
        if (sg) {
            if (sg->q) HIPCHK(h, hipMemcpyAsync(sg->q + (size_t)l * M * d.nq, q, M * d.nq * 4, hipMemcpyDeviceToDevice, st));
            if (sg->attn) HIPCHK(h, hipMemcpyAsync(sg->attn + (size_t)l * M * d.nq, att, M * d.nq * 4, hipMemcpyDeviceToDevice, st));
            if (sg->layer_out) HIPCHK(h, hipMemcpyAsync(sg->layer_out + (size_t)l * M * d.dim, x, M * d.dim * 4, hipMemcpyDeviceToDevice, st));
        }
    }
    if (sg && sg->final_norm) hipLaunchKernelGGL(lm_rmsnorm_kernel, dim3((unsigned)M), dim3(64), 0, st, s.hdr, x, h->blob + m.norm, d.dim, c.norm_eps, sg->final_norm);
    LmGemv hd{};
    hd.hdr = s.hdr; hd.x = x; hd.nw = h->blob + m.norm; hd.wa = h->blob + m.head; hd.K = d.dim; hd.N = d.C; hd.pairs = cdiv(d.C, 2); hd.eps = c.norm_eps;
    hd.heads = d.ncb;
    if (all_out) {
        for (int k = 0; k < d.ncb && k < T; ++k) {         // the rows i = k, k + ncb, ...: one head each
            hd.r = LmRows{B, cdiv(T - k, d.ncb), k, d.ncb, T};
            hd.out = all_out; hd.out_T = T; hd.out_ioff = 0;
            launch_gemv<LM_EPI_HEAD>(st, hd);
        }
    }
    hd.r = LmRows{B, 1, T - 1, 1, T};
    hd.out = s.pend; hd.out_T = 1; hd.out_ioff = T - 1;
    launch_gemv<LM_EPI_HEAD>(st, hd);
    return hipGetLastError() == hipSuccess ? AC_OK : fail(h, AC_EHIP, "a Llama decoder launch failed");
}

int lm_check(ac_handle* h, const char* what, const void* state, size_t state_bytes, int B, int cap, int max_steps) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->arch != ARCH_LM) return fail(h, AC_EINVAL, "%s: not a Llama decoder handle (ac_lm_create)", what);
    const LmDims d = lm_dims(h->lcfg);
    if (B < 1 || B > LM_MAX_ROWS) return fail(h, AC_EINVAL, "%s: %d rows per state (1..%d)", what, B, LM_MAX_ROWS);
    if (cap < 1 || cap > d.rows) return fail(h, AC_EINVAL, "%s: a capacity of %d positions (1..%d = 2 * max_seq_len, where the rotary table ends)", what, cap, d.rows);
    if (max_steps < 0 || max_steps > d.rows) return fail(h, AC_EINVAL, "%s: max_steps %d (0..%d)", what, max_steps, d.rows);
    if (!state || (reinterpret_cast<uintptr_t>(state) & 255)) return fail(h, AC_EINVAL, "%s: the state must be a 256-byte aligned device buffer", what);
    ac_lm_layout o;
    lm_layout(d, B, cap, max_steps, &o);
    if (state_bytes < (size_t)o.total) return fail(h, AC_ENOMEM, "%s: state too small: %zu < %lld bytes", what, state_bytes, o.total);
    return AC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// weight packing (the LlamaDecoder's state-dict keys; "lm.rope_cos" / "lm.rope_sin" are the caller's table)
// ---------------------------------------------------------------------------------------------
int lm_finalize(ac_handle* h, Packer& pk) {
    const ac_lm_config& c = h->lcfg;
    const LmDims d = lm_dims(c);
    LmPlan& m = h->lm;
    auto vec = [&](const std::string& name, size_t nel, size_t& off) {
        const std::vector<float>* v = pk.get(name, nel);
        if (!v) return false;
        off = pk.reserve(nel);
        std::copy(v->begin(), v->end(), pk.blob.begin() + off);
        return true;
    };
    if (!vec("tok_embeddings.weight", (size_t)d.ncb * d.C * d.dim, m.emb) || !vec("norm.weight", d.dim, m.norm)) return pk.rc;
    if (d.pd > 0 && !vec("prompt.weight", (size_t)d.dim * d.pd, m.prompt)) return pk.rc;
    if (d.ncb > 1) {                                    // output.k.weight stacked [ncb][C][dim]
        m.head = pk.reserve((size_t)d.ncb * d.C * d.dim);
        for (int k = 0; k < d.ncb; ++k) {
            const std::vector<float>* v = pk.get("output." + std::to_string(k) + ".weight", (size_t)d.C * d.dim);
            if (!v) return pk.rc;
            std::copy(v->begin(), v->end(), pk.blob.begin() + m.head + (size_t)k * d.C * d.dim);
        }
    } else if (!vec("output.weight", (size_t)d.C * d.dim, m.head)) {
        return pk.rc;
    }
    if (!vec("lm.rope_cos", (size_t)d.rows * (d.hd / 2), m.rope_cos) || !vec("lm.rope_sin", (size_t)d.rows * (d.hd / 2), m.rope_sin)) return pk.rc;
    m.layers.resize(d.L);
    for (int l = 0; l < d.L; ++l) {
        const std::string p = "layers." + std::to_string(l);
        LmLayer& ly = m.layers[l];
        const std::vector<float>* wq = pk.get(p + ".attention.wq.weight", (size_t)d.nq * d.dim);
        const std::vector<float>* wk = pk.get(p + ".attention.wk.weight", (size_t)d.nkvd * d.dim);
        const std::vector<float>* wv = pk.get(p + ".attention.wv.weight", (size_t)d.nkvd * d.dim);
        if (!wq || !wk || !wv) return pk.rc;
        ly.wqkv = pk.reserve((size_t)(d.nq + 2 * d.nkvd) * d.dim);
        std::copy(wq->begin(), wq->end(), pk.blob.begin() + ly.wqkv);
        std::copy(wk->begin(), wk->end(), pk.blob.begin() + ly.wqkv + (size_t)d.nq * d.dim);
        std::copy(wv->begin(), wv->end(), pk.blob.begin() + ly.wqkv + (size_t)(d.nq + d.nkvd) * d.dim);
        if (!vec(p + ".attention.wo.weight", (size_t)d.dim * d.nq, ly.wo) || !vec(p + ".attention_norm.weight", d.dim, ly.an) ||
            !vec(p + ".ffn_norm.weight", d.dim, ly.fn) || !vec(p + ".feed_forward.w1.weight", (size_t)d.ffn * d.dim, ly.w1) ||
            !vec(p + ".feed_forward.w3.weight", (size_t)d.ffn * d.dim, ly.w3) || !vec(p + ".feed_forward.w2.weight", (size_t)d.dim * d.ffn, ly.w2))
            return pk.rc;
    }
    return AC_OK;
}

}  // namespace acimpl

extern "C" {

int ac_lm_create(const ac_lm_config* cfg, ac_handle** out) {
    if (!cfg || !out) return AC_EINVAL;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(ac_lm_config)) return AC_EINVAL;
    const ac_lm_config& c = *cfg;
    if (c.n_layers < 1 || c.n_layers > 256 || c.dim < 4 || c.dim > 8192 || c.dim % 4 || c.ffn_dim < 4 || c.ffn_dim % 4) return AC_EINVAL;
    if (c.n_heads < 1 || c.dim % c.n_heads || c.n_kv_heads < 1 || c.n_heads % c.n_kv_heads) return AC_EINVAL;
    const int hd = c.dim / c.n_heads, group = c.n_heads / c.n_kv_heads;
    if (hd % 2 || hd > LM_MAX_HD) return AC_EINVAL;                                        // RoPE pairs; 4 elements per lane
    if (group != 1 && group != 2 && group != 4 && group != LM_MAX_GROUP) return AC_EINVAL;  // the attention kernel's instances
    if (c.vocab_size < 2 || c.vocab_size > 16384) return AC_EINVAL;                         // the sampler's range
    if (c.num_codebooks < 1 || c.num_codebooks > 64 || c.max_seq_len < 1 || c.max_seq_len > (1 << 20)) return AC_EINVAL;
    if (c.prompt_dim < 0 || c.prompt_dim % 4) return AC_EINVAL;
    if (!(c.norm_eps > 0.f) || !(c.rope_theta > 0.f)) return AC_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c.device || c.device < 0) return AC_ENODEV;
    ac_handle* h = new (std::nothrow) ac_handle();
    if (!h) return AC_ENOMEM;
    h->arch = ARCH_LM;
    h->lcfg = c;
    h->hop = 1;
    h->D = c.dim;
    *out = h;
    return AC_OK;
}

int ac_lm_state_layout(const ac_handle* h, int B, int capacity, int max_steps, ac_lm_layout* out) {
    if (!h || h->arch != ARCH_LM || !out || B < 1 || B > LM_MAX_ROWS || capacity < 1 || max_steps < 0) return AC_EINVAL;
    lm_layout(lm_dims(h->lcfg), B, capacity, max_steps, out);
    return AC_OK;
}

size_t ac_lm_state_bytes(const ac_handle* h, int B, int capacity, int max_steps) {
    ac_lm_layout o;
    return ac_lm_state_layout(h, B, capacity, max_steps, &o) == AC_OK ? (size_t)o.total : 0;
}

int ac_lm_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, int capacity, int max_steps, long long offset, void* stream) {
    int rc = lm_check(h, "ac_lm_reset", state_dev, state_bytes, B, capacity, max_steps);
    if (rc) return rc;
    if (offset < 0) return fail(h, AC_EINVAL, "ac_lm_reset: negative draw offset");
    const LmState s = lm_state(lm_dims(h->lcfg), state_dev, B, capacity, max_steps);
    hipLaunchKernelGGL(lm_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, LmInit{s.hdr, s.alive, s.lens, B, capacity, max_steps, offset});
    return hipGetLastError() == hipSuccess ? AC_OK : fail(h, AC_EHIP, "ac_lm_reset: launch failed");
}

size_t ac_lm_workspace_bytes(const ac_handle* h, int B, int T, int capacity) {
    if (!h || h->arch != ARCH_LM || B < 1 || B > LM_MAX_ROWS || T < 1 || capacity < 1) return 0;
    return lm_plan_ws(lm_dims(h->lcfg), B, T, capacity).total;
}

int ac_lm_embed(ac_handle* h, const int64_t* toks_dev, int B, int T, int curr_pos, const float* prompt_dev, int P, int prompt_width, float* out_dev, void* stream) {
    int rc = check_ready(h);
    if (rc) return rc;
    if (h->arch != ARCH_LM) return fail(h, AC_EINVAL, "ac_lm_embed: not a Llama decoder handle (ac_lm_create)");
    const LmDims d = lm_dims(h->lcfg);
    if (!out_dev || B < 1 || T < 0 || P < 0 || T + P < 1 || curr_pos < 0 || (T > 0 && !toks_dev) || (P > 0 && !prompt_dev))
        return fail(h, AC_EINVAL, "ac_lm_embed: bad argument (B=%d, T=%d, P=%d)", B, T, P);
    if ((long long)B * (T + P) > 0x7fffffffLL / 4) return fail(h, AC_EINVAL, "ac_lm_embed: too many rows");
    hipStream_t st = (hipStream_t)stream;
    if (P > 0) {
        if (prompt_width == d.dim && !(d.pd == d.dim)) {      // already in the model's width: prepended as it is
            HIPCHK(h, hipMemcpy2DAsync(out_dev, (size_t)(P + T) * d.dim * 4, prompt_dev, (size_t)P * d.dim * 4, (size_t)P * d.dim * 4, B, hipMemcpyDeviceToDevice, st));
        } else if (d.pd > 0 && prompt_width == d.pd) {
            LmGemv g{};
            g.x = prompt_dev; g.wa = h->blob + h->lm.prompt; g.K = d.pd; g.N = d.dim; g.pairs = d.dim / 2; g.r = LmRows{B, P, 0, 1, P};
            g.out = out_dev; g.out_T = P + T; g.out_ioff = 0;
            launch_gemv<LM_EPI_PLAIN>(st, g);
        } else {
            return fail(h, AC_EINVAL, "ac_lm_embed: prompt rows of width %d (prompt_dim %d, dim %d)", prompt_width, d.pd, d.dim);
        }
    }
    if (T > 0)
        hipLaunchKernelGGL(lm_embed_kernel, dim3((unsigned)(B * T)), dim3(256), 0, st, reinterpret_cast<const long long*>(toks_dev), B, T, h->blob + h->lm.emb, d.C, d.ncb,
                           d.dim, curr_pos, out_dev, P + T, P);
    return hipGetLastError() == hipSuccess ? AC_OK : fail(h, AC_EHIP, "ac_lm_embed: launch failed");
}

int ac_lm_forward(ac_handle* h, void* state_dev, size_t state_bytes, int B, int capacity, int max_steps, int pos, const float* embs_dev, int T,
                  float* logits_out, const ac_lm_stages* stages, void* ws, size_t ws_bytes, void* stream) {
    int rc = lm_check(h, "ac_lm_forward", state_dev, state_bytes, B, capacity, max_steps);
    if (rc) return rc;
    if (!embs_dev || T < 1 || pos < 0) return fail(h, AC_EINVAL, "ac_lm_forward: bad argument (T=%d, pos=%d)", T, pos);
    if ((long long)pos + T > capacity) return fail(h, AC_EINVAL, "ac_lm_forward: rows %d..%d pass the state's capacity of %d positions", pos, pos + T - 1, capacity);
    const LmDims d = lm_dims(h->lcfg);
    if ((long long)B * T * std::max(d.ffn, d.C) > 0x7fffffffLL) return fail(h, AC_EINVAL, "ac_lm_forward: %d rows are too many for one call: split them", T);
    if (!ws) return fail(h, AC_EINVAL, "workspace pointer is null");
    const LmWs w = lm_plan_ws(d, B, T, capacity);
    if (ws_bytes < w.total) return fail(h, AC_ENOMEM, "workspace too small: %zu < %zu bytes", ws_bytes, w.total);
    char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    const LmState s = lm_state(d, state_dev, B, capacity, max_steps);
    HIPCHK(h, hipMemcpyAsync(base + w.x, embs_dev, (size_t)B * T * d.dim * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(lm_begin_rows_kernel, dim3(1), dim3(1), 0, st, s.hdr, pos, T, B, capacity);
    return lm_layers(h, st, s, B, T, capacity, base, w, logits_out, stages);
}

int ac_lm_step(ac_handle* h, void* state_dev, size_t state_bytes, int B, int capacity, int max_steps, long long eos_id, float temp, float top_p,
               uint64_t key, float* logits_log, void* ws, size_t ws_bytes, void* stream) {
    int rc = lm_check(h, "ac_lm_step", state_dev, state_bytes, B, capacity, max_steps);
    if (rc) return rc;
    if (max_steps < 1) return fail(h, AC_EINVAL, "ac_lm_step: the state was laid out for no generated token (max_steps = 0)");
    if (!(temp > 0.f) || !std::isfinite(temp) || !(top_p >= 0.f) || !(top_p <= 1.f)) return fail(h, AC_EINVAL, "ac_lm_step: temp %g, top_p %g", (double)temp, (double)top_p);
    if (!ws) return fail(h, AC_EINVAL, "workspace pointer is null");
    const LmDims d = lm_dims(h->lcfg);
    const LmWs w = lm_plan_ws(d, B, 1, capacity);
    if (ws_bytes < w.total) return fail(h, AC_ENOMEM, "workspace too small: %zu < %zu bytes", ws_bytes, w.total);
    char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    const LmState s = lm_state(d, state_dev, B, capacity, max_steps);
    // the draw of row r: element (the state's offset word) + r of the stream; the word advances by B per recorded step
    rc = ac_sample_tokens(s.pend, d.C, nullptr, B, d.C, temp, 0, top_p, key, 0, reinterpret_cast<const int64_t*>(s.hdr + LMH_OFF), -1.0f, nullptr,
                          reinterpret_cast<int64_t*>(s.tok), stream);
    if (rc) return fail(h, rc, "ac_lm_step: the sampler refused the call");
    LmStep p{s.hdr, s.alive, s.lens, s.tok, s.hyp, s.pend, logits_log, h->blob + h->lm.emb, reinterpret_cast<float*>(base + w.x),
             B, d.C, d.C, d.ncb, d.dim, capacity, max_steps, eos_id};
    hipLaunchKernelGGL(lm_step_begin_kernel, dim3(1), dim3(256), 0, st, p);
    return lm_layers(h, st, s, B, 1, capacity, base, w, nullptr, nullptr);
}

}  // extern "C"
