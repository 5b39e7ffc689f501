// probe_path.hip: the TokenProbe -- the downstream recipes' probe over codec tokens: MultiHeadEmbedding and
// Linear / Attentional pooling fused into one gather (probe.h), a bidirectional LSTM over packed sequences with one plain launch per step
// (bilstm.h), and a CTC head with greedy collapse or an utterance head over masked statistics pooling (probe.h).  The input projections
// and the CTC head are linear_rows (split16 on the fp16 matrix pipe, per-row scales).  The launch sequence of a chunk of clips is one
// linear chain of plain launches: zero fill, pool, then per layer one projection and N steps, then the head.
#include "core.h"
#include "probe.h"

namespace acimpl {

namespace {

constexpr size_t PB_WS_CAP = (size_t)1 << 30;         // workspace cap that sizes the chunk of clips ac_probe_workspace_bytes plans for
constexpr int PB_MAX_CLIPS = 4096;                    // clips per pass at most
constexpr int PB_MAX_H = 1024, PB_MAX_LAYERS = 8;

struct PbDims {
    int K, C, E, H, L, NC, pool, head, pad, trows;    // trows: rows of the embedding table
};

PbDims pb_dims(const ac_probe_config& c) {
    PbDims d;
    d.K = c.num_codebooks; d.C = c.vocab_size; d.E = c.embedding_dim; d.H = c.hidden_size; d.L = c.num_layers; d.NC = c.num_classes;
    d.pool = c.pooling; d.head = c.head; d.pad = c.padding_idx ? 1 : 0; d.trows = d.K * d.C + d.pad;
    return d;
}

int pb_cpad(const PbDims& d) { return (d.NC + 63) / 64 * 64; }      // the CTC head's rows as Packer::pack6 packs them

// the layout of a pass over Bc clips of N frames (byte offsets): the split16 pool, x (pooled), gin, then the zero-filled region -- every
// layer's output, the two h buffers and c -- and the logits
struct PbWs {
    int Bc = 0, Bpad = 0;
    size_t pool = 0, x = 0, gin = 0, zero = 0, zero_bytes = 0, y = 0, y_layer = 0, hbuf = 0, hbuf_one = 0, c = 0, logits = 0, total = 0;
};

PbWs pb_plan_ws(const PbDims& d, int Bc, int N) {
    PbWs w;
    w.Bc = Bc;
    w.Bpad = (Bc + 31) / 32 * 32;
    const size_t rows = (size_t)Bc * N;
    size_t o = align_up(pool_bytes(Bc, rows), 256);
    auto take = [&](size_t floats) { const size_t at = o; o += align_up(floats * 4, 256); return at; };
    w.x = take(d.pool != AC_PROBE_POOL_NONE ? rows * d.E : 0);
    w.gin = take(rows * 8 * d.H);
    w.zero = o;
    w.y_layer = align_up(rows * 2 * d.H * 4, 256);
    w.y = o;
    o += w.y_layer * d.L;
    w.hbuf_one = align_up((size_t)2 * w.Bpad * d.H * 4, 256);
    w.hbuf = o;
    o += 2 * w.hbuf_one;
    w.c = take((size_t)2 * w.Bpad * d.H);
    w.zero_bytes = o - w.zero;
    w.logits = take(d.head == AC_PROBE_HEAD_CTC ? rows * pb_cpad(d) : (size_t)Bc * d.NC);
    w.total = o + 512;
    return w;
}

// clips per pass under the cap (at least one)
int pb_cap_clips(const PbDims& d, int B, int N) {
    const size_t per = pb_plan_ws(d, 32, N).total / 32 + 1;
    return (int)std::min<size_t>((size_t)std::min(B, PB_MAX_CLIPS), std::max<size_t>(1, PB_WS_CAP / per));
}

unsigned grid1d(long long n, int per) { return (unsigned)std::max<long long>(1, std::min<long long>((n + per - 1) / per, 65535LL * 16)); }

int stage_copy(ac_handle* h, hipStream_t st, float* dst, const float* src, long long rows, int width, int pitch) {
    if (!dst) return AC_OK;
    HIPCHK(h, hipMemcpy2DAsync(dst, (size_t)width * 4, src, (size_t)pitch * 4, (size_t)width * 4, (size_t)rows, hipMemcpyDeviceToDevice, st));
    return AC_OK;
}

int launch_step(ac_handle* h, hipStream_t st, const BiLstmStep& p, int H) {
    const dim3 grid((unsigned)(H / 4), (unsigned)(p.Bpad / 32), 2u), block(256);
#define PB_STEP(KS) case KS: hipLaunchKernelGGL((bilstm_step_kernel<KS>), grid, block, 0, st, p); break;
    switch (H / 32) {
        PB_STEP(1) PB_STEP(2) PB_STEP(4) PB_STEP(8) PB_STEP(16)
        default: return fail(h, AC_EINVAL, "hidden_size %d has no recurrence kernel (32, 64, 128, 256, 512)", H);
    }
#undef PB_STEP
    return AC_OK;
}

bool pb_has_step(int H) { return H == 32 || H == 64 || H == 128 || H == 256 || H == 512; }

// nb clips of N frames; the output pointers arrive advanced to the chunk's first clip, `Ball` is the call's batch (layer pitch of a stage)
int pb_chunk_fwd(ac_handle* h, hipStream_t st, const void* input, int nb, int N, const long long* lengths, const ac_probe_outputs& o, int Ball, char* base,
                 const PbWs& w) {
    const PbDims d = pb_dims(h->pcfg);
    const ProbePlan& m = h->probe;
    const long long rows = (long long)nb * N;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    int rc;
    hipLaunchKernelGGL(probe_zero_kernel, dim3(grid1d((long long)(w.zero_bytes / 16), 256 * 4)), dim3(256), 0, st, reinterpret_cast<s16_f32x4*>(base + w.zero),
                       (long long)(w.zero_bytes / 16));
    HIPCHK(h, hipGetLastError());
    const float* x = reinterpret_cast<const float*>(input);
    const unsigned* words = nullptr;
    int width = d.E;
    if (d.pool != AC_PROBE_POOL_NONE) {
        unsigned* rw = rowmax_new(h, st, rows, false);
        if (!rw) return fail(h, AC_ENOMEM, "the workspace pool's row ring is too small for %lld rows", rows);
        ProbeEmbedPool p{};
        p.toks = reinterpret_cast<const long long*>(input);
        p.table = h->blob + m.table;
        p.wlin = d.pool == AC_PROBE_POOL_LINEAR && d.K > 1 ? h->blob + m.wlin : nullptr;
        p.score = d.pool == AC_PROBE_POOL_ATTENTIONAL ? h->blob + m.score : nullptr;
        p.out = F(w.x); p.rowmax = rw; p.bad = h->sticky_dev ? h->sticky_dev + ST_BAD_TOKEN : nullptr;
        p.rows = rows; p.K = d.K; p.C = d.C; p.E = d.E; p.padding = d.pad;
        ProfScope ps(h, st, "probe_embed_pool_kernel", 2.0 * rows * d.K * d.E, 4.0 * rows * (d.K + 1) * d.E);
        hipLaunchKernelGGL(probe_embed_pool_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, p);
        HIPCHK(h, hipGetLastError());
        if ((rc = stage_copy(h, st, o.pooled, F(w.x), rows, d.E, d.E))) return rc;
        x = F(w.x);
        words = rw;
    }
    float* gin = F(w.gin);
    for (int l = 0; l < d.L; ++l) {
        Epi e;
        e.rowmax_in = words;
        if ((rc = linear_rows(h, st, m.ih[l], x, rows, width, width, 0, gin, 8 * d.H, e))) return rc;
        float* y = reinterpret_cast<float*>(base + w.y + (size_t)l * w.y_layer);
        {
            ProfScope ps(h, st, "bilstm_step_kernel", 2.0 * 2 * N * (double)nb * 4 * d.H * d.H, 2.0 * N * 4.0 * 4 * d.H * d.H, N);
            for (int s = 0; s < N; ++s) {
                BiLstmStep p{};
                p.gin = gin; p.wpk = h->blob + m.hh[l];
                p.hprev = reinterpret_cast<const float*>(base + w.hbuf + (size_t)((s + 1) & 1) * w.hbuf_one);
                p.hnext = reinterpret_cast<float*>(base + w.hbuf + (size_t)(s & 1) * w.hbuf_one);
                p.c = F(w.c); p.y = y; p.lengths = lengths; p.B = nb; p.Bpad = w.Bpad; p.N = N; p.s = s;
                if ((rc = launch_step(h, st, p, d.H))) return rc;
            }
            HIPCHK(h, hipGetLastError());
        }
        if ((rc = stage_copy(h, st, o.layer_out ? o.layer_out + (size_t)l * Ball * N * 2 * d.H : nullptr, y, rows, 2 * d.H, 2 * d.H))) return rc;
        x = y;
        width = 2 * d.H;
        words = nullptr;                                    // (the tap-GEMM reads the rows' amax itself: one more launch per layer)
    }
    if (d.head == AC_PROBE_HEAD_CTC) {
        const int cpad = m.cpad;
        float* lg = F(w.logits);
        if ((rc = linear_rows(h, st, m.head, x, rows, 2 * d.H, 2 * d.H, 0, lg, cpad))) return rc;
        if ((rc = stage_copy(h, st, o.logits, lg, rows, d.NC, cpad))) return rc;
        hipLaunchKernelGGL(probe_ctc_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st,
                           ProbeCtcRows{lg, lengths, reinterpret_cast<long long*>(o.frame_pred), o.log_probs, nb, N, d.NC, cpad});
        hipLaunchKernelGGL(probe_ctc_collapse_kernel, dim3((unsigned)nb), dim3(256), 0, st,
                           ProbeCollapse{reinterpret_cast<const long long*>(o.frame_pred), reinterpret_cast<long long*>(o.hyp_toks),
                                         reinterpret_cast<long long*>(o.hyp_lens), N, (long long)h->pcfg.blank_id});
    } else {
        const size_t lds = probe_utt_lds(2 * d.H);
        hipLaunchKernelGGL(probe_utt_head_kernel, dim3((unsigned)nb), dim3(256), lds, st,
                           ProbeUttHead{x, lengths, h->blob + m.head_w, h->blob + m.head_b, F(w.logits), o.logits, o.log_probs, reinterpret_cast<long long*>(o.pred), N,
                                        2 * d.H, d.NC});
    }
    HIPCHK(h, hipGetLastError());
    return AC_OK;
}

int pb_check(ac_handle* h, const char* what) {
    if (int rc = check_ready(h)) return rc;
    if (h->arch != ARCH_PROBE) return fail(h, AC_EINVAL, "%s: not a token-probe handle (ac_probe_create)", what);
    return AC_OK;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// weight packing (torch's names; "pooling.score" is the caller's fold of AttentionalPooling's MLP)
// ---------------------------------------------------------------------------------------------
int probe_finalize(ac_handle* h, Packer& pk) {
    const PbDims d = pb_dims(h->pcfg);
    ProbePlan& m = h->probe;
    if (h->gemm_fp32)
        return fail(h, AC_EINVAL, "a token probe runs its input projections in split16 arithmetic only (precision \"fp32\"); exact-product mode has no row-mode GEMM");
    auto vec = [&](const std::string& name, size_t nel, size_t& off) {
        const std::vector<float>* v = pk.get(name, nel);
        if (!v) return false;
        off = pk.reserve(nel);
        std::copy(v->begin(), v->end(), pk.blob.begin() + off);
        return true;
    };
    if (d.pool != AC_PROBE_POOL_NONE && !vec("embedding.weight", (size_t)d.trows * d.E, m.table)) return pk.rc;
    if (d.pool == AC_PROBE_POOL_LINEAR && d.K > 1 && !vec("pooling.mlp.weight", d.K, m.wlin)) return pk.rc;
    if (d.pool == AC_PROBE_POOL_ATTENTIONAL && !vec("pooling.score", (size_t)d.K * d.C + 2, m.score)) return pk.rc;
    const int H = d.H;
    m.ih.resize(d.L);
    m.hh.resize(d.L);
    for (int l = 0; l < d.L; ++l) {
        const int in = l == 0 ? d.E : 2 * H;
        PackedGemm& g = m.ih[l];
        g.N = 8 * H;
        g.Ktot = in;
        g.has_bias = true;
        g.w_off = pk.reserve((size_t)8 * H * in);
        g.b_off = pk.reserve((size_t)8 * H);
        m.hh[l] = pk.reserve((size_t)2 * 4 * H * H);
        for (int dir = 0; dir < 2; ++dir) {
            const std::string sfx = "_l" + std::to_string(l) + (dir ? "_reverse" : "");
            const std::vector<float>* wih = pk.get("encoder.rnn.weight_ih" + sfx, (size_t)4 * H * in);
            const std::vector<float>* whh = pk.get("encoder.rnn.weight_hh" + sfx, (size_t)4 * H * H);
            const std::vector<float>* bih = pk.get("encoder.rnn.bias_ih" + sfx, (size_t)4 * H);
            const std::vector<float>* bhh = pk.get("encoder.rnn.bias_hh" + sfx, (size_t)4 * H);
            if (!wih || !whh || !bih || !bhh) return pk.rc;
            std::copy(wih->begin(), wih->end(), pk.blob.begin() + g.w_off + (size_t)dir * 4 * H * in);
            for (int n = 0; n < 4 * H; ++n) pk.blob[g.b_off + (size_t)dir * 4 * H + n] = (*bih)[n] + (*bhh)[n];
            // W_hh in MFMA B-fragment order (Packer::lstm): [ug][k-step][lane][u] = Whh[(j >> 2) H + 4 ug + (j & 3)][16 ks + 4 kq + u]
            const size_t off = m.hh[l] + (size_t)dir * 4 * H * H;
            for (int ug = 0; ug < H / 4; ++ug)
                for (int ks = 0; ks < H / 16; ++ks)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int u = 0; u < 4; ++u) {
                            const int j = lane & 15, kq = lane >> 4;
                            const int row = (j >> 2) * H + ug * 4 + (j & 3);
                            const int k = ks * 16 + 4 * kq + u;
                            pk.blob[off + (((size_t)ug * (H / 16) + ks) * 64 + lane) * 4 + u] = (*whh)[(size_t)row * H + k];
                        }
        }
        pk.pack6(g);
        if (!h->w6_of.count(g.w_off) || !h->winv_of.count(g.w_off)) return fail(h, AC_EINVAL, "layer %d's input projection [%d][%d] was not packed for the matrix pipe", l, 8 * H, in);
    }
    if (d.head == AC_PROBE_HEAD_CTC) {
        const std::vector<float>* w = pk.get("head.weight", (size_t)d.NC * 2 * H);
        const std::vector<float>* b = pk.get("head.bias", (size_t)d.NC);
        if (!w || !b) return pk.rc;
        PackedGemm& g = m.head;
        m.cpad = pb_cpad(d);
        g.N = m.cpad;
        g.Ktot = 2 * H;
        g.has_bias = true;
        g.w_off = pk.reserve((size_t)m.cpad * 2 * H);       // (reserve zero-fills: the padding rows and their biases are zero)
        g.b_off = pk.reserve((size_t)m.cpad);
        std::copy(w->begin(), w->end(), pk.blob.begin() + g.w_off);
        std::copy(b->begin(), b->end(), pk.blob.begin() + g.b_off);
        pk.pack6(g);
        if (!h->w6_of.count(g.w_off) || !h->winv_of.count(g.w_off)) return fail(h, AC_EINVAL, "the CTC head [%d][%d] was not packed for the matrix pipe", m.cpad, 2 * H);
    } else {
        if (!vec("head.weight", (size_t)d.NC * 4 * H, m.head_w) || !vec("head.bias", (size_t)d.NC, m.head_b)) return pk.rc;
    }
    return AC_OK;
}

}  // namespace acimpl

extern "C" {

int ac_probe_create(const ac_probe_config* cfg, ac_handle** out) {
    if (!cfg || !out) return AC_EINVAL;
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(ac_probe_config)) return AC_EINVAL;
    const ac_probe_config& c = *cfg;
    if (c.pooling != AC_PROBE_POOL_NONE && c.pooling != AC_PROBE_POOL_LINEAR && c.pooling != AC_PROBE_POOL_ATTENTIONAL) return AC_EINVAL;
    if (c.head != AC_PROBE_HEAD_CTC && c.head != AC_PROBE_HEAD_UTTERANCE) return AC_EINVAL;
    if (c.hidden_size < 32 || c.hidden_size > PB_MAX_H || c.hidden_size % 32 || !pb_has_step(c.hidden_size)) return AC_EINVAL;
    if (c.embedding_dim < 32 || c.embedding_dim > 8192 || c.embedding_dim % 32) return AC_EINVAL;      // what Packer::pack6 packs
    if (c.num_layers < 1 || c.num_layers > PB_MAX_LAYERS || c.num_classes < 1 || c.num_classes > 65536) return AC_EINVAL;
    if (c.pooling != AC_PROBE_POOL_NONE) {
        if (c.num_codebooks < 1 || c.num_codebooks > PROBE_MAX_K || c.vocab_size < 1 || c.vocab_size > (1 << 20)) return AC_EINVAL;
    }
    if (c.head == AC_PROBE_HEAD_CTC && (c.blank_id < 0 || c.blank_id >= c.num_classes)) return AC_EINVAL;
    if (c.padding_idx != 0 && c.padding_idx != 1) return AC_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c.device || c.device < 0) return AC_ENODEV;
    ac_handle* h = new (std::nothrow) ac_handle();
    if (!h) return AC_ENOMEM;
    h->arch = ARCH_PROBE;
    h->pcfg = c;
    h->hop = 1;
    h->D = c.hidden_size;
    *out = h;
    return AC_OK;
}

size_t ac_probe_workspace_bytes(const ac_handle* h, int B, int N) {
    if (!h || h->arch != ARCH_PROBE || B < 1 || N < 1) return 0;
    const PbDims d = pb_dims(h->pcfg);
    return pb_plan_ws(d, pb_cap_clips(d, B, N), N).total;
}

int ac_probe_forward(ac_handle* h, const void* input_dev, int B, int N, const int64_t* lengths_dev, const ac_probe_outputs* out, void* ws, size_t ws_bytes,
                     void* stream) {
    if (int rc = pb_check(h, "ac_probe_forward")) return rc;
    const PbDims d = pb_dims(h->pcfg);
    if (!input_dev || !out || B < 1 || N < 1) return fail(h, AC_EINVAL, "ac_probe_forward: bad argument (B=%d, N=%d)", B, N);
    if (d.head == AC_PROBE_HEAD_CTC && (!out->frame_pred || !out->hyp_toks || !out->hyp_lens))
        return fail(h, AC_EINVAL, "ac_probe_forward: a CTC head writes frame_pred, hyp_toks and hyp_lens");
    if (d.head == AC_PROBE_HEAD_UTTERANCE && (!out->log_probs || !out->pred)) return fail(h, AC_EINVAL, "ac_probe_forward: an utterance head writes log_probs and pred");
    if (!aligned16(input_dev)) return fail(h, AC_EINVAL, "ac_probe_forward: the input must be 16-byte aligned");
    if (!ws) return fail(h, AC_EINVAL, "workspace pointer is null");
    if (d.head == AC_PROBE_HEAD_UTTERANCE)
        if (int rc = ensure_lds(h, reinterpret_cast<const void*>(probe_utt_head_kernel), probe_utt_lds(2 * d.H))) return rc;
    // the clips of a pass: as many as the workspace at hand holds (ac_probe_workspace_bytes plans for the capped number)
    int Bc = std::min(B, PB_MAX_CLIPS);
    while (Bc > 0 && pb_plan_ws(d, Bc, N).total > ws_bytes) --Bc;
    if (Bc < 1) return fail(h, AC_ENOMEM, "workspace too small: %zu < %zu bytes (one clip)", ws_bytes, pb_plan_ws(d, 1, N).total);
    const PbWs w = pb_plan_ws(d, Bc, N);
    char* base = reinterpret_cast<char*>(align_up(reinterpret_cast<uintptr_t>(ws), 256));
    hipStream_t st = (hipStream_t)stream;
    const long long* lengths = reinterpret_cast<const long long*>(lengths_dev);
    const size_t in_clip = d.pool != AC_PROBE_POOL_NONE ? (size_t)N * d.K * 8 : (size_t)N * d.E * 4;      // bytes of one clip of the input
    for (int b0 = 0; b0 < B; b0 += Bc) {
        const int nb = std::min(Bc, B - b0);
        pool_bind(h, base, Bc, (size_t)Bc * N);
        if (int rc = amax_begin(h, st, nb)) return rc;
        const size_t r0 = (size_t)b0 * N;
        ac_probe_outputs o{};
        const bool ctc = d.head == AC_PROBE_HEAD_CTC;
        o.frame_pred = out->frame_pred ? out->frame_pred + r0 : nullptr;
        o.hyp_toks = out->hyp_toks ? out->hyp_toks + r0 : nullptr;
        o.hyp_lens = out->hyp_lens ? out->hyp_lens + b0 : nullptr;
        o.log_probs = out->log_probs ? out->log_probs + (ctc ? r0 * d.NC : (size_t)b0 * d.NC) : nullptr;
        o.pred = out->pred ? out->pred + b0 : nullptr;
        o.pooled = out->pooled && d.pool != AC_PROBE_POOL_NONE ? out->pooled + r0 * d.E : nullptr;
        o.layer_out = out->layer_out ? out->layer_out + r0 * 2 * d.H : nullptr;
        o.logits = out->logits ? out->logits + (ctc ? r0 * d.NC : (size_t)b0 * d.NC) : nullptr;
        if (int rc = pb_chunk_fwd(h, st, reinterpret_cast<const char*>(input_dev) + (size_t)b0 * in_clip, nb, N, lengths ? lengths + b0 : nullptr, o, B, base, w))
            return rc;
    }
    return AC_OK;
}

}  // extern "C"
