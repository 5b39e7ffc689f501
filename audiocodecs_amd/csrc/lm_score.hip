// lm_score.hip: the full-sequence Llama forward that scores token sequences (llama_score.h) -- the packing of the
// layer matrices for the matrix pipe (ac_lm_prepare_score), the workspace of a chunk of clips, the launch sequence of one chunk and the
// ac_lm_score* entry points.  Every matrix product is linear_rows (split16 on the fp16 matrix pipe, per-row scales); the decode step's
// fp32 matrices (lm_path.hip) stay where they are and ac_lm_forward / ac_lm_step do not change.
#include "core.h"
#include "llama_score.h"

namespace acimpl {

namespace {

constexpr size_t LS_WS_CAP = (size_t)1 << 30;         // workspace cap that sizes the chunk of clips ac_lm_score_workspace_bytes plans for
constexpr int LS_MAX_CLIPS = 4096;                    // clips per pass at most (the pool has 64 KB of amax slots per clip)
constexpr int LS_MAX_DIM = 2048;                      // the head kernel keeps 16 rows of `dim` as two fp16 planes in LDS

struct LsDims {
    int L, dim, ffn, nh, nkv, hd, nq, nkvd, nqkv, C, ncb, rows;
};

LsDims ls_dims(const ac_lm_config& c) {
    LsDims d;
    d.L = c.n_layers; d.dim = c.dim; d.ffn = c.ffn_dim; d.nh = c.n_heads; d.nkv = c.n_kv_heads; d.hd = c.dim / c.n_heads;
    d.nq = d.nh * d.hd; d.nkvd = d.nkv * d.hd; d.nqkv = d.nq + 2 * d.nkvd; d.C = c.vocab_size; d.ncb = c.num_codebooks; d.rows = 2 * c.max_seq_len;
    return d;
}

// the layout of a pass over Bc clips of Ttot rows: the split16 pool, then x | n | qkv | att | h2 | hid, each Bc times its per-clip size
struct LsWs {
    int Bc = 0;
    size_t pool = 0, x = 0, n = 0, qkv = 0, att = 0, h2 = 0, hid = 0, total = 0;
};

size_t ls_clip_bytes(const LsDims& d, int Ttot, LsWs* w) {
    size_t o = 0;
    auto take = [&](size_t* dst, size_t floats) { if (dst) *dst = o; o += align_up(floats * 4, 256); };
    take(w ? &w->x : nullptr, (size_t)Ttot * d.dim);
    take(w ? &w->n : nullptr, (size_t)Ttot * d.dim);
    take(w ? &w->qkv : nullptr, (size_t)Ttot * d.nqkv);
    take(w ? &w->att : nullptr, (size_t)Ttot * d.nq);
    take(w ? &w->h2 : nullptr, (size_t)Ttot * 2 * d.ffn);
    take(w ? &w->hid : nullptr, (size_t)Ttot * d.ffn);
    return o;
}

LsWs ls_plan_ws(const LsDims& d, int Bc, int Ttot) {
    LsWs w;
    const size_t per = ls_clip_bytes(d, Ttot, &w);
    w.Bc = Bc;
    w.pool = align_up(pool_bytes(Bc, (size_t)Bc * Ttot), 256);
    size_t* offs[] = {&w.x, &w.n, &w.qkv, &w.att, &w.h2, &w.hid};
    for (size_t* o : offs) *o = w.pool + *o * (size_t)Bc;
    w.total = w.pool + per * (size_t)Bc + 512;
    return w;
}

// clips per pass under the cap (at least one)
int ls_cap_clips(const LsDims& d, int B, int Ttot) {
    const size_t per = ls_clip_bytes(d, Ttot, nullptr);
    return (int)std::min<size_t>((size_t)std::min(B, LS_MAX_CLIPS), std::max<size_t>(1, LS_WS_CAP / std::max<size_t>(per, 1)));
}

unsigned grid1d(long long n, int per) { return (unsigned)std::max<long long>(1, std::min<long long>((n + per - 1) / per, 65535LL * 16)); }

int launch_attn(ac_handle* h, hipStream_t st, const LmAttn16& p, int hd, int clips, int nkv) {
    const dim3 grid((unsigned)cdiv(p.T, 16), (unsigned)nkv, (unsigned)clips), block(64 * p.G);
#define LS_ATTN(HD)                                                                                                       \
    case HD: {                                                                                                            \
        if (int rc = ensure_lds(h, reinterpret_cast<const void*>(lm_attn16_causal_kernel<HD>), LmAttn16Cfg<HD>::lds_bytes)) return rc; \
        hipLaunchKernelGGL((lm_attn16_causal_kernel<HD>), grid, block, LmAttn16Cfg<HD>::lds_bytes, st, p);                \
        break;                                                                                                            \
    }
    switch (hd) {
        LS_ATTN(16) LS_ATTN(32) LS_ATTN(48) LS_ATTN(64) LS_ATTN(80) LS_ATTN(96) LS_ATTN(112) LS_ATTN(128)
        default: return fail(h, AC_EINVAL, "head dim %d has no causal attention kernel (multiples of 16 up to 128)", hd);
    }
#undef LS_ATTN
    return AC_OK;
}

// rows [r0, r0 + rows) of a [.][pitch] matrix, `width` floats each, to a dense [rows][width] stage buffer
int stage_copy(ac_handle* h, hipStream_t st, float* dst, const float* src, long long rows, int width, int pitch) {
    if (!dst) return AC_OK;
    HIPCHK(h, hipMemcpy2DAsync(dst, (size_t)width * 4, src, (size_t)pitch * 4, (size_t)width * 4, (size_t)rows, hipMemcpyDeviceToDevice, st));
    return AC_OK;
}

// nb clips: embs [nb][Ttot][dim]; the stage pointers arrive advanced to the chunk's first clip, `Ball` is the call's batch (layer pitch)
int ls_chunk_fwd(ac_handle* h, hipStream_t st, const float* embs, int nb, int P, int T, const long long* targets, const long long* lengths, float* logp,
                 long long* pred, const ac_lm_score_stages& sg, int Ball, char* base, const LsWs& w) {
    const ac_lm_config& c = h->lcfg;
    const LsDims d = ls_dims(c);
    const LmPlan& m = h->lm;
    const int Ttot = P + T;
    const long long rows = (long long)nb * Ttot;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    float *x = F(w.x), *n = F(w.n), *qkv = F(w.qkv), *att = F(w.att), *h2 = F(w.h2), *hid = F(w.hid);
    int rc;
    hipLaunchKernelGGL(lm_copy4_kernel, dim3(grid1d(rows * d.dim / 4, 256 * 4)), dim3(256), 0, st, reinterpret_cast<const ls_f32x4*>(embs),
                       reinterpret_cast<ls_f32x4*>(x), rows * d.dim / 4);
    auto norm = [&](size_t w_off, const unsigned** words) -> int {
        unsigned* rw = nullptr;
        if (words) {
            rw = rowmax_new(h, st, rows, false);
            if (!rw) return fail(h, AC_ENOMEM, "the workspace pool's row ring is too small for %lld rows", rows);
            *words = rw;
        }
        hipLaunchKernelGGL(lm_norm_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, LmNormRows{x, h->blob + w_off, n, rw, rows, d.dim, c.norm_eps});
        HIPCHK(h, hipGetLastError());
        return AC_OK;
    };
    const long long lp = (long long)Ball * Ttot;            // rows of one layer in a stage buffer
    for (int l = 0; l < d.L; ++l) {
        const LmLayer& ly = m.layers[l];
        const unsigned* words = nullptr;
        if ((rc = norm(ly.an, &words))) return rc;
        Epi eq;
        eq.rowmax_in = words;
        if ((rc = linear_rows(h, st, ly.g_qkv, n, rows, d.dim, d.dim, 0, qkv, d.nqkv, eq))) return rc;
        hipLaunchKernelGGL(lm_rope_rows_kernel, dim3((unsigned)rows), dim3(256), 0, st,
                           LmRopeRows{qkv, h->blob + m.rope_cos, h->blob + m.rope_sin, Ttot, d.nqkv, d.nq + d.nkvd, d.hd});
        HIPCHK(h, hipGetLastError());
        if ((rc = stage_copy(h, st, sg.q ? sg.q + l * lp * d.nq : nullptr, qkv, rows, d.nq, d.nqkv))) return rc;
        if ((rc = stage_copy(h, st, sg.k ? sg.k + l * lp * d.nkvd : nullptr, qkv + d.nq, rows, d.nkvd, d.nqkv))) return rc;
        {
            const LmAttn16 a{qkv, att, Ttot, d.nqkv, d.nq, d.nkvd, d.nh / d.nkv, 1.0f / std::sqrt((float)d.hd)};
            ProfScope ps(h, st, "lm_attn16_causal_kernel", 6.0 * nb * d.nh * (double)Ttot * Ttot * d.hd, 4.0 * rows * (d.nqkv + d.nq));
            if ((rc = launch_attn(h, st, a, d.hd, nb, d.nkv))) return rc;
            HIPCHK(h, hipGetLastError());
        }
        if ((rc = stage_copy(h, st, sg.attn ? sg.attn + l * lp * d.nq : nullptr, att, rows, d.nq, d.nq))) return rc;
        Epi ea;
        ea.res = x;
        ea.res_rs = d.dim;
        if ((rc = linear_rows(h, st, ly.g_o, att, rows, d.nq, d.nq, 0, x, d.dim, ea))) return rc;
        if ((rc = norm(ly.fn, &words))) return rc;
        Epi eg;
        eg.rowmax_in = words;
        if ((rc = linear_rows(h, st, ly.g_13, n, rows, d.dim, d.dim, 0, h2, 2 * d.ffn, eg))) return rc;
        unsigned* hw = rowmax_new(h, st, rows, false);
        if (!hw) return fail(h, AC_ENOMEM, "the workspace pool's row ring is too small for %lld rows", rows);
        hipLaunchKernelGGL(lm_swiglu_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, LmSwigluRows{h2, hid, hw, rows, d.ffn});
        HIPCHK(h, hipGetLastError());
        Epi em;
        em.rowmax_in = hw;
        em.res = x;
        em.res_rs = d.dim;
        if ((rc = linear_rows(h, st, ly.g_2, hid, rows, d.ffn, d.ffn, 0, x, d.dim, em))) return rc;
        if ((rc = stage_copy(h, st, sg.layer_out ? sg.layer_out + l * lp * d.dim : nullptr, x, rows, d.dim, d.dim))) return rc;
    }
    if ((rc = norm(m.norm, nullptr))) return rc;
    if ((rc = stage_copy(h, st, sg.final_norm, n, rows, d.dim, d.dim))) return rc;
    const size_t lds = lm_score_head_lds(m.head_ksteps);
    if ((rc = ensure_lds(h, reinterpret_cast<const void*>(lm_score_head_kernel), lds))) return rc;
    for (int k = 0; k < d.ncb && k < T; ++k) {             // the positions t = k, k + ncb, ...: one head each (P is a multiple of ncb)
        LmScoreHead p{};
        p.xn = n;
        p.img = reinterpret_cast<const _Float16*>(h->blob + m.head_img) + (size_t)k * m.head_cpad * m.head_ksteps * 64;   // (2 planes x 32 dims per row and k-step)
        p.winv = h->blob + m.head_inv + (size_t)k * m.head_cpad;
        p.targets = targets; p.lengths = lengths; p.logp = logp; p.pred = pred; p.logits = sg.logits;
        p.clips = nb; p.T = T; p.P = P; p.dim = d.dim; p.C = d.C; p.ncb = d.ncb; p.k = k; p.KS = m.head_ksteps; p.ntiles = m.head_cpad / 16;
        p.Tk = cdiv(T - k, d.ncb);
        const long long Mk = (long long)nb * p.Tk;
        ProfScope ps(h, st, "lm_score_head_kernel", 6.0 * Mk * d.C * (double)d.dim, 4.0 * Mk * d.dim + 4.0 * (double)d.C * d.dim);
        hipLaunchKernelGGL(lm_score_head_kernel, dim3((unsigned)((Mk + LSH_ROWS - 1) / LSH_ROWS)), dim3(256), lds, st, p);
        HIPCHK(h, hipGetLastError());
    }
    return AC_OK;
}

int ls_check(ac_handle* h, const char* what) {
    if (int rc = check_ready(h)) return rc;
    if (h->arch != ARCH_LM) return fail(h, AC_EINVAL, "%s: not a Llama decoder handle (ac_lm_create)", what);
    return AC_OK;
}

}  // namespace

}  // namespace acimpl

extern "C" {

int ac_lm_prepare_score(ac_handle* h) {
    if (int rc = ls_check(h, "ac_lm_prepare_score")) return rc;
    LmPlan& m = h->lm;
    if (m.score_ready) return AC_OK;
    const LsDims d = ls_dims(h->lcfg);
    if (h->gemm_fp32) return fail(h, AC_EINVAL, "ac_lm_prepare_score: the scoring forward runs in split16 arithmetic only (precision \"fp32\")");
    auto fits = [](int N, int K) { return (N % 64 == 0 || N % 96 == 0) && K % 32 == 0; };      // what Packer::pack6 packs for the tap-GEMM
    if (!fits(d.nqkv, d.dim) || !fits(d.dim, d.nq) || !fits(2 * d.ffn, d.dim) || !fits(d.dim, d.ffn))
        return fail(h, AC_EINVAL, "ac_lm_prepare_score: the layer matrices ([%d][%d], [%d][%d], [%d][%d], [%d][%d]) need rows in multiples of 64 or 96 and columns in "
                    "multiples of 32 for the matrix pipe", d.nqkv, d.dim, d.dim, d.nq, 2 * d.ffn, d.dim, d.dim, d.ffn);
    if (d.hd % 16 || d.hd > 128) return fail(h, AC_EINVAL, "ac_lm_prepare_score: head dim %d (the causal attention has multiples of 16 up to 128)", d.hd);
    if (d.dim > LS_MAX_DIM) return fail(h, AC_EINVAL, "ac_lm_prepare_score: dim %d exceeds the head kernel's limit of %d", d.dim, LS_MAX_DIM);
    // the blob comes back to the host once, gains the images, and is uploaded again: every offset into it stays valid
    HIPCHK(h, hipSetDevice(h->lcfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    Packer pk{h};
    pk.blob.resize(h->blob_floats);
    HIPCHK(h, hipMemcpy(pk.blob.data(), h->blob, h->blob_floats * sizeof(float), hipMemcpyDeviceToHost));
    auto gemm = [&](PackedGemm& g, size_t w_off, int N, int K) {
        g.w_off = w_off; g.b_off = 0; g.N = N; g.Ktot = K; g.has_bias = false;
        pk.pack6(g);
        return h->w6_of.count(w_off) != 0 && h->winv_of.count(w_off) != 0;
    };
    for (int l = 0; l < d.L; ++l) {
        LmLayer& ly = m.layers[l];
        const size_t w13 = pk.reserve((size_t)2 * d.ffn * d.dim);
        std::copy(pk.blob.begin() + ly.w1, pk.blob.begin() + ly.w1 + (size_t)d.ffn * d.dim, pk.blob.begin() + w13);
        std::copy(pk.blob.begin() + ly.w3, pk.blob.begin() + ly.w3 + (size_t)d.ffn * d.dim, pk.blob.begin() + w13 + (size_t)d.ffn * d.dim);
        if (!gemm(ly.g_qkv, ly.wqkv, d.nqkv, d.dim) || !gemm(ly.g_o, ly.wo, d.dim, d.nq) || !gemm(ly.g_13, w13, 2 * d.ffn, d.dim) || !gemm(ly.g_2, ly.w2, d.dim, d.ffn))
            return fail(h, AC_ESTATE, "ac_lm_prepare_score: layer %d was not packed", l);
    }
    {   // the heads, each padded to whole tiles of 16 columns (zero rows) and whole k-steps of 32 (zero columns)
        const int cpad = (d.C + 15) / 16 * 16, ks = (d.dim + 31) / 32;
        const size_t src = pk.reserve((size_t)d.ncb * cpad * d.dim);
        for (int k = 0; k < d.ncb; ++k)
            std::copy(pk.blob.begin() + m.head + (size_t)k * d.C * d.dim, pk.blob.begin() + m.head + (size_t)(k + 1) * d.C * d.dim,
                      pk.blob.begin() + src + (size_t)k * cpad * d.dim);
        std::vector<int> km((size_t)ks * 32);
        for (int i = 0; i < ks * 32; ++i) km[i] = i < d.dim ? i : -1;
        m.head_img = pk.frag16(src, d.ncb * cpad, d.dim, km, &m.head_inv);
        m.head_cpad = cpad;
        m.head_ksteps = ks;
    }
    float* fresh = nullptr;
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&fresh), pk.blob.size() * sizeof(float)));
    if (hipMemcpy(fresh, pk.blob.data(), pk.blob.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(fresh);
        return fail(h, AC_EHIP, "ac_lm_prepare_score: the upload failed");
    }
    (void)hipFree(h->blob);
    h->blob = fresh;
    h->blob_floats = pk.blob.size();
    m.score_ready = true;
    return AC_OK;
}

size_t ac_lm_score_workspace_bytes(const ac_handle* h, int B, int T_total) {
    if (!h || h->arch != ARCH_LM || B < 1 || T_total < 1) return 0;
    const LsDims d = ls_dims(h->lcfg);
    return ls_plan_ws(d, ls_cap_clips(d, B, T_total), T_total).total;
}

int ac_lm_score(ac_handle* h, const float* embs_dev, int B, int P, int T, const int64_t* targets_dev, const int64_t* lengths_dev, float* logp_out, int64_t* pred_out,
                double* sum_logp_out, int64_t* count_out, int64_t* errors_out, const ac_lm_score_stages* stages, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = ls_check(h, "ac_lm_score")) return rc;
    if (!h->lm.score_ready) return fail(h, AC_ESTATE, "ac_lm_score: ac_lm_prepare_score has not been called");
    const LsDims d = ls_dims(h->lcfg);
    if (!embs_dev || !targets_dev || !logp_out || !pred_out || !sum_logp_out || !count_out || !errors_out || B < 1 || P < 0 || T < 1)
        return fail(h, AC_EINVAL, "ac_lm_score: bad argument (B=%d, P=%d, T=%d)", B, P, T);
    if ((long long)P + T > d.rows) return fail(h, AC_EINVAL, "ac_lm_score: %lld rows pass 2 * max_seq_len = %d, where the rotary table ends", (long long)P + T, d.rows);
    if (P % d.ncb) return fail(h, AC_EINVAL, "ac_lm_score: a prompt of %d rows is no multiple of num_codebooks (%d)", P, d.ncb);
    if (!ws) return fail(h, AC_EINVAL, "workspace pointer is null");
    const int Ttot = P + T;
    // the clips of a pass: as many as the workspace at hand holds (ac_lm_score_workspace_bytes plans for the capped number)
    int Bc = std::min(B, LS_MAX_CLIPS);
    while (Bc > 0 && ls_plan_ws(d, Bc, Ttot).total > ws_bytes) --Bc;
    if (Bc < 1) return fail(h, AC_ENOMEM, "workspace too small: %zu < %zu bytes (one clip)", ws_bytes, ls_plan_ws(d, 1, Ttot).total);
    if ((long long)Bc * Ttot * std::max(2 * d.ffn, d.C) > 0x7fffffffLL) Bc = (int)std::max<long long>(1, 0x7fffffffLL / ((long long)Ttot * std::max(2 * d.ffn, d.C)));
    const LsWs w = ls_plan_ws(d, Bc, Ttot);
    char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    const long long* targets = reinterpret_cast<const long long*>(targets_dev);
    const long long* lengths = reinterpret_cast<const long long*>(lengths_dev);
    long long* pred = reinterpret_cast<long long*>(pred_out);
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        pool_bind(h, base, Bc, (size_t)Bc * Ttot);
        if (int rc = amax_begin(h, st, nb)) return rc;
        ac_lm_score_stages sg{};
        if (stages) {
            const size_t r0 = (size_t)b0 * Ttot;
            sg.q = stages->q ? stages->q + r0 * d.nq : nullptr;
            sg.k = stages->k ? stages->k + r0 * d.nkvd : nullptr;
            sg.attn = stages->attn ? stages->attn + r0 * d.nq : nullptr;
            sg.layer_out = stages->layer_out ? stages->layer_out + r0 * d.dim : nullptr;
            sg.final_norm = stages->final_norm ? stages->final_norm + r0 * d.dim : nullptr;
            sg.logits = stages->logits ? stages->logits + (size_t)b0 * T * d.C : nullptr;
        }
        if (int rc = ls_chunk_fwd(h, st, embs_dev + (size_t)b0 * Ttot * d.dim, nb, P, T, targets + (size_t)b0 * T, lengths ? lengths + b0 : nullptr,
                                  logp_out + (size_t)b0 * T, pred + (size_t)b0 * T, sg, B, base, w))
            return rc;
    }
    hipLaunchKernelGGL(lm_score_reduce_kernel, dim3((unsigned)B), dim3(256), 0, st,
                       LmScoreReduce{logp_out, pred, targets, lengths, sum_logp_out, reinterpret_cast<long long*>(count_out), reinterpret_cast<long long*>(errors_out), T, d.C});
    return hipGetLastError() == hipSuccess ? AC_OK : fail(h, AC_EHIP, "ac_lm_score: a launch failed");
}

}  // extern "C"
