/*
 * audiocodecs_amd.h -- C ABI of the MI355X (gfx950) EnCodec encode/decode path.
 *
 * Drop-in boundary: the reference is pure Python and has no FFI of its own; the calls this
 * library replaces are the third-party model calls inside the reference wrapper
 *     audiocodecs/encodec.py:90-93   self.model.encode(sig[:, None], padding_mask[:, None], bandwidth)
 *     audiocodecs/encodec.py:139-140 self.model.decode(toks[None].movedim(-1, -2), [None])
 *     audiocodecs/encodec.py:116     self.model.encoder(input_values)            (_sig_to_feats)
 *     audiocodecs/encodec.py:125,147 self.model.quantizer.decode(toks)           (_sig_to_qfeats/_toks_to_qfeats)
 *     audiocodecs/encodec.py:74-79   quantizer.layers[k].codebook.embed           (embs)
 * which sit behind Codec.sig_to_toks / toks_to_sig / sig_to_feats / toks_to_qfeats / embs
 * (audiocodecs/codec.py:57-107,182-184).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *  - plain pointers and sizes only; every *_dev pointer is HIP device memory owned by the caller;
 *  - all work is enqueued on the caller's `stream` (a hipStream_t passed as void*); no entry point
 *    synchronises the device, so the caller's own fences (torch.cuda.synchronize in
 *    downstream/test_sr.py:58,84) time the real work;
 *  - no compute entry point allocates or frees device memory: every byte a call needs beyond the handle's weights
 *    (activations, LSTM state, and the split-operand bookkeeping -- per-clip amax slots and the per-row ring) is carved
 *    from the caller's workspace, whose size ac_encode_workspace_bytes / ac_decode_workspace_bytes /
 *    ac_quantizer_workspace_bytes report for the call's (B, T | N); B may grow or shrink from call to call without any
 *    hipMalloc / hipFree / stream synchronisation inside the library (tests/test_workspace_contract_gpu.py).  The handle
 *    owns only what ac_finalize allocates once: the packed weights, the persistent LSTM's control words, a pinned status
 *    word, and (Mimi) a few KB of pool for ac_embs_projected, the one launching entry point without a workspace argument;
 *  - return 0 on success, a negative AC_E* code on failure; never throws across the ABI;
 *    ac_last_error() returns a human-readable message for the last failure on that handle;
 *  - a handle is not thread-safe; one handle per process/GPU like the reference's one codec/rank;
 *    the handle's device (ac_config.device) must be the current HIP device when its entry points run;
 *  - activations, weights and results are fp32, accumulation is fp32, tokens are int64 like the reference's.  The
 *    large GEMMs, the fused residual blocks and the LSTM products run "split-operand" arithmetic on the fp16 matrix pipe:
 *    every fp32 operand, scaled by a power of two, is written as two fp16 terms and 3 of the 4 exact partial products
 *    are accumulated in fp32 (fp32-grade error: K = 1536 dot products measure 1.9e-7 rms against an fp32 FMA chain's
 *    1.8e-7).  ac_set_precision selects the one alternative: exact fp32 products
 *    (v_mfma_f32_16x16x4_f32) in every kernel.  (The three-bf16-term and rounded-bf16 modes of rounds 1-3 are gone;
 *    their values are rejected.)
 */
#ifndef AUDIOCODECS_AMD_H
#define AUDIOCODECS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AC_OK 0
#define AC_EINVAL (-1)   /* bad argument / shape / unsupported configuration            */
#define AC_ESTATE (-2)   /* call order (weights missing, not finalized, ...)             */
#define AC_ENOMEM (-3)   /* device allocation failed or workspace too small              */
#define AC_EHIP (-4)     /* a HIP runtime call or kernel launch failed                   */
#define AC_ENODEV (-5)   /* no gfx950 device visible                                     */

#define AC_MAX_RATIOS 8

typedef struct ac_handle ac_handle;

/* Mirrors the fields of transformers.EncodecConfig the path depends on.
 * Causal convs, reflect padding, weight-norm (pre-folded), mono, no chunking, normalize=False:
 * the facebook/encodec_24khz variant the reference wrapper loads (encodec.py:49-51). */
typedef struct ac_config {
    int32_t struct_size;               /* = sizeof(ac_config)                                  */
    int32_t sampling_rate;             /* 24000                                                */
    int32_t num_filters;               /* 32                                                   */
    int32_t hidden_size;               /* 128 (latent width == codebook dim)                   */
    int32_t num_ratios;                /* 4                                                    */
    int32_t upsampling_ratios[AC_MAX_RATIOS]; /* 8,5,4,2 (decoder order; encoder uses reverse) */
    int32_t kernel_size;               /* 7                                                    */
    int32_t last_kernel_size;          /* 7                                                    */
    int32_t residual_kernel_size;      /* 3                                                    */
    int32_t compress;                  /* 2                                                    */
    int32_t num_lstm_layers;           /* 2                                                    */
    int32_t codebook_size;             /* 1024                                                 */
    int32_t num_quantizers;            /* 32                                                   */
    int32_t device;                    /* HIP device ordinal                                   */
} ac_config;

/* Mimi: the fields of transformers.MimiConfig the path depends on; defaults = kyutai/mimi,
 * what audiocodecs/mimi.py:45 loads.  Replaces, behind Mimi._sig_to_toks/_toks_to_sig/_sig_to_feats/
 * _toks_to_qfeats/embs (mimi.py:52-156):
 *     mimi.py:105-108  self.model.encode(sig[:, None], padding_mask[:, None], num_quantizers=K)
 *     mimi.py:146-147  self.model.decode(toks.movedim(-1, -2))
 *     mimi.py:115-119  encoder -> encoder_transformer -> downsample
 *     mimi.py:139,153  self.model.quantizer.decode(...)
 * Causal convs with zero ("constant") padding, identity ResBlock shortcuts, no weight-norm, multi-head
 * attention with num_key_value_heads == num_attention_heads, "default" RoPE, exact-erf GELU, LayerScale. */
typedef struct ac_mimi_config {
    int32_t struct_size;               /* = sizeof(ac_mimi_config)                              */
    int32_t sampling_rate;             /* 24000                                                 */
    int32_t num_filters;               /* 64                                                    */
    int32_t hidden_size;               /* 512 (transformer / latent width)                      */
    int32_t num_ratios;                /* 4                                                     */
    int32_t upsampling_ratios[AC_MAX_RATIOS]; /* 8,6,5,4 (decoder order)                        */
    int32_t kernel_size;               /* 7                                                     */
    int32_t last_kernel_size;          /* 3                                                     */
    int32_t residual_kernel_size;      /* 3                                                     */
    int32_t compress;                  /* 2                                                     */
    int32_t codebook_size;             /* 2048                                                  */
    int32_t codebook_dim;              /* 256 (== vector_quantization_hidden_dimension)         */
    int32_t num_quantizers;            /* 32                                                    */
    int32_t num_semantic_quantizers;   /* 1                                                     */
    int32_t num_hidden_layers;         /* 8 (per transformer)                                   */
    int32_t num_attention_heads;       /* 8                                                     */
    int32_t head_dim;                  /* 64                                                    */
    int32_t intermediate_size;         /* 2048                                                  */
    int32_t sliding_window;            /* 250                                                   */
    int32_t resample_stride;           /* 2 (encodec_frame_rate / frame_rate)                   */
    int32_t device;                    /* HIP device ordinal                                    */
    float rope_theta;                  /* 10000                                                 */
    float norm_eps;                    /* 1e-5                                                  */
} ac_mimi_config;

/* DAC (BASELINE.json configs[2]).  The reference wrapper (audiocodecs/dac.py:28-130) calls
 * `dac.DAC` of descript-audio-codec 1.0.0, which is NOT on disk: parity with it is unpinned; this path is
 * pinned to the same-architecture transformers.DacModel (field names below are DacConfig's).  Replaces
 *     dac.py:96-99    self.model.encode(sig[:, None], n_quantizers=K)            -> ac_encode / ac_encode_quantized
 *     dac.py:105-111  self.model.encoder(...), quantizers[0].in_proj(...)          -> ac_encode_feats / ac_encode_feats_latent
 *     dac.py:126-129  self.model.quantizer.from_codes(...), self.model.decode(...) -> ac_decode (ac_dequantize_ws)
 *     dac.py:63-90    codebooks / out_proj(codebooks)                              -> ac_embs / ac_embs_projected */
#define AC_MAX_DILATIONS 4
typedef struct ac_dac_config {
    int32_t struct_size;               /* = sizeof(ac_dac_config)                               */
    int32_t sampling_rate;             /* 44100                                                 */
    int32_t encoder_hidden_size;       /* 64                                                    */
    int32_t decoder_hidden_size;       /* 1536                                                  */
    int32_t num_ratios;                /* 4                                                     */
    int32_t downsampling_ratios[AC_MAX_RATIOS]; /* 2,4,8,8                                      */
    int32_t upsampling_ratios[AC_MAX_RATIOS];   /* 8,8,4,2                                      */
    int32_t n_codebooks;               /* 9                                                     */
    int32_t codebook_size;             /* 1024                                                  */
    int32_t codebook_dim;              /* 8 (the only supported value)                          */
    int32_t num_dilations;             /* 3 residual units per block ...                        */
    int32_t dilations[AC_MAX_DILATIONS]; /* ... with dilations 1,3,9                            */
    int32_t device;
} ac_dac_config;

/* WavTokenizer (BASELINE.json configs[4]).  The reference wrapper (audiocodecs/wavtokenizer.py:31-135)
 * calls the package `wavtokenizer` (lucadellalib/WavTokenizer), which is NOT on disk: PARITY UNPINNED -- this path is
 * pinned to oracle/wavtokenizer_oracle.py, a restatement of the published modules.  Replaces
 *     wavtokenizer.py:94-95    self.model.encode(sig, bandwidth_id=0)                  -> ac_encode (K = 1) / ac_dequantize
 *     wavtokenizer.py:101      self.model.feature_extractor.encodec.encoder(sig[:, None]) -> ac_encode_feats
 *     wavtokenizer.py:115-118  codes_to_features(...) + self.model.decode(feats, bandwidth_id=0) -> ac_decode (ac_dequantize)
 *     wavtokenizer.py:130-133  self.model.decode(feats.movedim(-1,-2), bandwidth_id=0)  -> ac_decode_feats
 *     wavtokenizer.py:87       quantizer.vq.layers[0].codebook                          -> ac_embs
 * Fields: the published YAML configs the wrapper names (:37-40).  Weight names are the checkpoint's own
 * ("feature_extractor.encodec.encoder.model.{i}.conv.conv.{weight_g,weight_v,bias}", "...block.{1,3}...", "...shortcut...",
 * "...model.{i}.lstm.weight_ih_l0", "feature_extractor.encodec.quantizer.vq.layers.0._codebook.embed",
 * "backbone.embed.*", "backbone.pos_net.{0,1,3,4}.{norm1,conv1,norm2,conv2}.*", "backbone.pos_net.2.{norm,q,k,v,proj_out}.*",
 * "backbone.pos_net.5.*", "backbone.norm.{scale,shift}.weight", "backbone.convnext.{l}.{dwconv,norm.scale,norm.shift,
 * pwconv1,pwconv2}.*", "...gamma", "backbone.final_layer_norm.*", "head.out.*", optional "head.istft.window"). */
typedef struct ac_wavtok_config {
    int32_t struct_size;               /* = sizeof(ac_wavtok_config)                                          */
    int32_t sampling_rate;             /* 24000                                                               */
    int32_t num_filters;               /* 32                                                                  */
    int32_t dimension;                 /* 512: encoder output width == codebook dim == backbone input width   */
    int32_t num_ratios;                /* 4                                                                   */
    int32_t ratios[AC_MAX_RATIOS];     /* 6,5,5,4 (`dowmsamples`; the encoder applies them reversed); 75 tok/s: 8,5,4,2 */
    int32_t kernel_size;               /* 7                                                                   */
    int32_t last_kernel_size;          /* 7                                                                   */
    int32_t residual_kernel_size;      /* 3                                                                   */
    int32_t compress;                  /* 2                                                                   */
    int32_t num_lstm_layers;           /* 2                                                                   */
    int32_t codebook_size;             /* 4096                                                                */
    int32_t backbone_dim;              /* 768 (256 also supported)                                            */
    int32_t intermediate_dim;          /* 2304                                                                */
    int32_t num_layers;                /* 12 ConvNeXt blocks                                                  */
    int32_t adanorm_num_embeddings;    /* 4                                                                   */
    int32_t num_groups;                /* 32 (GroupNorm of pos_net)                                           */
    int32_t n_fft;                     /* 2400 (hop 600); 1280 (hop 320); must be a multiple of the hop       */
    int32_t bandwidth_id;              /* 0: the AdaLayerNorm row the wrapper always selects                  */
    int32_t device;
} ac_wavtok_config;

/* Vocos decoder for EnCodec tokens (the reference's Encodec(use_vocos=True), audiocodecs/encodec.py:53-66,130-138, loads
 * charactr/vocos-encodec-24khz through the package `vocos`, which is NOT on disk: PARITY UNPINNED -- this path is pinned to a
 * restatement of the published Vocos 0.1.0 modules, tests/vocos_ref.py over oracle/wavtokenizer_oracle.py).  Replaces
 *     encodec.py:133-137   vocos.codes_to_features(toks) + vocos.decode(feats, bandwidth_id=...)   -> ac_decode
 * A decode-only handle: WavTokenizer's decoder without pos_net.  ac_decode(toks [B,N,K]) sums rows toks[..,k] + k*codebook_size of
 * "feature_extractor.codebook_weights" [max_codebooks*codebook_size, input_channels] for the K the CALL gives (1..max_codebooks),
 * then "backbone.embed.*" (Conv1d k7), "backbone.norm.{scale,shift}.weight" (AdaLayerNorm, row bandwidth_id),
 * "backbone.convnext.{l}.{dwconv,norm.scale,norm.shift,pwconv1,pwconv2}.*" + "...gamma", "backbone.final_layer_norm.*",
 * "head.out.*" and the inverse STFT ("same" padding; optional "head.istft.window", periodic Hann when absent).  Every other key is
 * ignored.  Serves ac_load_weights, ac_set_precision, ac_finalize, ac_decode_workspace_bytes, ac_decode, ac_dequantize (the
 * summed features), ac_embs (the tables), ac_poll_status, ac_debug_capture, ac_profile_*, ac_hop_length, ac_destroy; the
 * encode-side calls fail ("without encoder weights"). */
typedef struct ac_vocos_config {
    int32_t struct_size;               /* = sizeof(ac_vocos_config)                                           */
    int32_t input_channels;            /* 128: width of a code vector == EnCodec's hidden_size                */
    int32_t codebook_size;             /* 1024                                                                */
    int32_t max_codebooks;             /* 16 tables in codebook_weights                                       */
    int32_t backbone_dim;              /* 384 (a multiple of 64, at most 1024)                                */
    int32_t intermediate_dim;          /* 1152                                                                */
    int32_t num_layers;                /* 8 ConvNeXt blocks                                                   */
    int32_t adanorm_num_embeddings;    /* 4: bandwidths 1.5, 3, 6, 12 kbps                                    */
    int32_t n_fft;                     /* 1280; a multiple of hop_length                                      */
    int32_t hop_length;                /* 320                                                                 */
    int32_t bandwidth_id;              /* the AdaLayerNorm row: [1.5, 3.0, 6.0, 12.0].index(bandwidth)        */
    int32_t device;
} ac_vocos_config;

/* Library/ABI version: major*10000 + minor*100 + patch. */
int ac_version(void);

/* Create a handle for `cfg` on device cfg->device.  No device memory is allocated yet. */
int ac_create(const ac_config* cfg, ac_handle** out);

/* Same, for a Mimi handle.  Every other entry point below works on either kind of handle. */
int ac_mimi_create(const ac_mimi_config* cfg, ac_handle** out);

/* Same, for a DAC handle (keys of DacModel.state_dict(): "encoder.conv1.weight", "encoder.block.{i}.
 * res_unit{u}.{snake1.alpha,conv1.weight,...}", "decoder.block.{i}.conv_t1.weight", "quantizer.quantizers.{k}.
 * {in_proj,out_proj}.{weight,bias}", "...codebook.weight"; weights plain, i.e. weight-norm already folded). */
int ac_dac_create(const ac_dac_config* cfg, ac_handle** out);

/* Same, for a WavTokenizer handle. */
int ac_wavtok_create(const ac_wavtok_config* cfg, ac_handle** out);

/* Same, for a Vocos-for-EnCodec decoder handle (decode only). */
int ac_vocos_create(const ac_vocos_config* cfg, ac_handle** out);

/* Hand one fp32 tensor to the handle (copied).  `name` uses the HF state-dict keys of
 * EncodecModel with weight-norm either
 *   - already folded:   "<prefix>.weight"  (what the Python host passes; folded with the same torch
 *                        primitive the reference's parametrisation evaluates), or
 *   - unfolded:         "<prefix>.parametrizations.weight.original0" (g) and "...original1" (v);
 *                        folded inside ac_finalize as  w = v * (g / ||v||_2), norm over dims (1,2).
 * plus "<prefix>.bias", "<lstm>.weight_{ih,hh}_l{n}", "<lstm>.bias_{ih,hh}_l{n}",
 * "quantizer.layers.{k}.codebook.embed".  Other keys (embed_avg, cluster_size, inited) are
 * accepted and ignored.  `bytes` must equal 4 * number of elements expected for that key.
 * Mimi handles take the keys of MimiModel.state_dict(): "<conv>.weight"/".bias" (no weight-norm),
 * "{encoder,decoder}_transformer.layers.{l}.{self_attn.{q,k,v,o}_proj,mlp.fc{1,2}}.weight",
 * ".{input,post_attention}_layernorm.{weight,bias}", ".{self_attn,mlp}_layer_scale.scale",
 * "downsample.conv.weight", "upsample.conv.weight",
 * "quantizer.{semantic,acoustic}_residual_vector_quantizer.{input,output}_proj.weight" and
 * "...layers.{q}.codebook.{embed_sum,cluster_usage}" (embed = embed_sum / max(cluster_usage, 1e-5),
 * [HF] mimi :980-983); optionally "encoder_transformer.rotary_emb.inv_freq" (the model's non-persistent
 * buffer; computed as 1/theta^(2i/d) in fp32 when absent). */
int ac_load_weights(ac_handle* h, const char* name, const void* host_ptr, size_t bytes);

/* Arithmetic of the GEMM-shaped kernels; call before ac_finalize (weights are packed for one arithmetic).
 *   AC_PRECISION_FP32        default: fp32 fidelity on the fp16 matrix pipe ("split16", csrc/split16.h): every operand as two
 *                            scaled fp16 planes (x 2^s = hi + lo, both round-to-nearest), 3 partial products, fp32 accumulate;
 *                            power-of-two scales per clip (activations: largest magnitude reported by the producing kernel), per
 *                            row (linear layers over merged token matrices) and per output channel (weights) -- the arithmetic
 *                            every parity claim is made for;
 *   AC_PRECISION_FP32_EXACT  exact fp32 products (v_mfma_f32_16x16x4_f32) everywhere; same as AC_GEMM=fp32;
 * (Rounds 1-3 also carried a three-bf16-plane arithmetic and an opt-in rounded-bf16 side mode; both were removed in round 4: neither
 * had a user, and the side mode kept fp32 activations in HBM -- no parity and no bandwidth saving.  Values 2 and 3 are rejected.)
 * Without this call the environment variable AC_GEMM=fp32 selects the exact-product kernels, default AC_PRECISION_FP32. */
#define AC_PRECISION_FP32 0
#define AC_PRECISION_FP32_EXACT 1
int ac_set_precision(ac_handle* h, int precision);

/* Check that every tensor of the configuration arrived, fold/pack them into the kernels' layouts
 * and upload them (one device allocation owned by the handle). */
int ac_finalize(ac_handle* h);

/* Frames produced for T samples: ceil at every strided conv (T=1..320 -> 1, 321 -> 2, ...). */
int ac_num_frames(const ac_handle* h, int T);
/* Samples ac_decode writes per clip for N frames: N*hop, except DAC (symmetric padding):
 * each transposed conv gives (L-1)*s - 2*ceil(s/2) + 2s.  DAC's ac_num_frames follows the strided convs
 * floor((L + 2*ceil(s/2) - 2s)/s) + 1 and is 0 when the input is too short (upstream's conv1d raises). */
long long ac_num_samples(const ac_handle* h, int N);
/* Hop length (product of ratios, 320; Mimi: x resample_stride = 1920), latent width of feats/qfeats
 * (128; Mimi 512) and codebook vector width (EnCodec: == hidden; Mimi 256). */
int ac_hop_length(const ac_handle* h);
int ac_hidden_size(const ac_handle* h);
int ac_codebook_dim(const ac_handle* h);

/* Scratch the caller must provide (device memory, 256-byte aligned) for one call. */
size_t ac_encode_workspace_bytes(const ac_handle* h, int B, int T);
size_t ac_decode_workspace_bytes(const ac_handle* h, int B, int N);

/* sig_dev [B,T] fp32  ->  toks_dev [B,N,K] int64,  N = ac_num_frames(T).
 * rel_len_dev: NULL, or [B] fp32 relative lengths (SpeechBrain style): sample t of clip b is
 * zeroed before the encoder iff not (float)t < (float)T * rel_len[b]   (encodec.py:84-89,
 * [HF] modeling_encodec.py:589-590).  Tokens are produced for all N frames regardless.
 * K = number of codebooks (quantizer stages), 1 <= K <= num_quantizers.
 * One clip per call is limited to 7 340 031 samples (DAC handles: 3 670 015): per-clip activations are addressed with
 * 32-bit byte offsets; longer clips return AC_EINVAL ("split it") -- the codecs are causal / chunkable on the host. */
int ac_encode(ac_handle* h, const float* sig_dev, const float* rel_len_dev, int B, int T, int K,
              int64_t* toks_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Encoder only: sig_dev [B,T] -> feats_dev [B,N,H] fp32 (channels-last, i.e. the wrapper's
 * `feats.movedim(-1,-2)` layout, encodec.py:116-118).  rel_len_dev as in ac_encode (the reference's
 * _sig_to_feats does not mask for the 24 kHz model: pass NULL to reproduce it). */
int ac_encode_feats(ac_handle* h, const float* sig_dev, const float* rel_len_dev, int B, int T,
                    float* feats_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* toks_dev [B,N,K] int64 (any ids in [0, codebook_size)) -> sig_dev [B, N*hop] fp32.
 * The output is not trimmed to the encoder's input length (encodec.py:139-140). */
int ac_decode(ac_handle* h, const int64_t* toks_dev, int B, int N, int K, float* sig_dev,
              void* workspace_dev, size_t workspace_bytes, void* stream);

/* WavTokenizer only (wavtokenizer.py:128-135 `_feats_to_sig`): feats_dev [B,N,dimension] (channels-last) -> sig_dev [B, N*hop]
 * through backbone + iSTFT head.  Workspace: ac_decode_workspace_bytes(h, B, N). */
int ac_decode_feats(ac_handle* h, const float* feats_dev, int B, int N, float* sig_dev, void* workspace_dev, size_t workspace_bytes,
                    void* stream);

/* DAC only.  ac_encode_quantized: ac_encode that also returns the quantised representation
 * qfeats_dev [B,N,H] `model.encode` yields (dac.py:117-119; not bit-identical to from_codes: the
 * straight-through form rounds).  ac_encode_feats_latent: quantizers[0].in_proj(encoder(sig)) -> [B,N,8]
 * (dac.py:104-108, `latent=True`). */
int ac_encode_quantized(ac_handle* h, const float* sig_dev, int B, int T, int K, int64_t* toks_dev, float* qfeats_dev,
                        void* workspace_dev, size_t workspace_bytes, void* stream);
int ac_encode_feats_latent(ac_handle* h, const float* sig_dev, int B, int T, float* feats_latent_dev,
                           void* workspace_dev, size_t workspace_bytes, void* stream);

/* RVQ only.  ac_quantize: feats_dev [B,N,H] -> toks_dev [B,N,K] ([HF]:424-438).
 * ac_dequantize: toks_dev [B,N,K] -> qfeats_dev [B,N,H] = sum_k E_k[tok]  ([HF]:440-447). */
int ac_quantize(ac_handle* h, const float* feats_dev, int B, int N, int K, int64_t* toks_dev, void* stream);
int ac_dequantize(ac_handle* h, const int64_t* toks_dev, int B, int N, int K, float* qfeats_dev, void* stream);
/* Mimi's split quantiser projects in and out of the codebook space (mimi.py:139,153 ->
 * [HF] mimi :1129-1138), which needs scratch: same calls with a workspace of
 * ac_quantizer_workspace_bytes(h, B, N) bytes (0 for EnCodec handles, which may pass NULL). */
size_t ac_quantizer_workspace_bytes(const ac_handle* h, int B, int N);
int ac_quantize_ws(ac_handle* h, const float* feats_dev, int B, int N, int K, int64_t* toks_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);
int ac_dequantize_ws(ac_handle* h, const int64_t* toks_dev, int B, int N, int K, float* qfeats_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* Streaming Mimi encode: B streams, F whole frames (F * hop samples) per stream and push; tokens [B,F,K] in ac_encode's layout.
 * The caller owns the stream state as device memory (ac_mimi_stream_state_bytes(h, B) bytes, 256-byte aligned), as it owns
 * workspaces: per stream the padding cache of every causal conv of the encoder and of the down-sampler, a K/V ring of the last
 * sliding_window - 1 positions per transformer layer, the absolute position and a "fresh" flag (DESIGN.md "Streaming Mimi encode").
 * ac_mimi_stream_reset marks the streams of reset_mask_dev [B] (NULL: all) fresh at position 0; the rings are not cleared (entries
 * from before a reset are masked by position).  A state must be reset on the handle, for the B it is used with, before its first
 * ac_mimi_stream_encode, and its first reset takes no mask.  Returns AC_EINVAL for a non-Mimi handle, a state this handle never
 * reset or reset for another B (the handle knows the states it reset by their address: memory reused at a reset state's address
 * passes as that state), and AC_ENOMEM for a state or workspace (ac_mimi_stream_workspace_bytes(h, B, F)) that is too
 * small; the handle stays usable.  Positions run up to 2^24 (the fp32 RoPE angle); no entry point allocates or synchronises. */
size_t ac_mimi_stream_state_bytes(const ac_handle* h, int B);
int ac_mimi_stream_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream);
size_t ac_mimi_stream_workspace_bytes(const ac_handle* h, int B, int F);
int ac_mimi_stream_encode(ac_handle* h, void* state_dev, size_t state_bytes, const float* sig_dev, int B, int F, int K,
                          int64_t* toks_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Streaming Mimi decode: B streams, F token frames per stream and push; toks_dev [B,F,K] in ac_decode's layout, sig_dev [B, F * hop]
 * fp32.  Decoding a stream frame by frame gives what ac_decode gives on the whole token sequence (the decoder is causal), for any
 * number of frames: positions are not bounded by ac_decode's RoPE table.  Same contract as the encode side: the caller owns the
 * state (ac_mimi_stream_decode_state_bytes(h, B) bytes, 256-byte aligned) and the workspace
 * (ac_mimi_stream_decode_workspace_bytes(h, B, F)); nothing allocates or synchronises.  Per stream the state holds the up-sampler's
 * previous input row, a K/V ring per layer of the decoder transformer (positions advance resample_stride per frame), the padding
 * cache of the first conv, of every transposed conv (its previous input row) and residual block, and of the head conv, the position
 * and the "fresh" flag (DESIGN.md "Streaming Mimi decode").  A decode state is NOT an encode state: it has its own layout and header
 * and the handle registers it as such -- an encode state passed to ac_mimi_stream_decode / _decode_reset (masked), or a decode state
 * passed to ac_mimi_stream_encode, is AC_EINVAL; resetting a buffer as one kind ends its life as the other.  AC_ESTATE for a handle
 * loaded without decoder weights; AC_EINVAL / AC_ENOMEM otherwise as for the encode side, decided on the host, and the handle and the
 * state stay usable.  Token ids outside [0, codebook_size) behave as in ac_decode: the frame is NaN (and what follows it in that
 * stream, through the state) and the NEXT entry point returns AC_EINVAL. */
size_t ac_mimi_stream_decode_state_bytes(const ac_handle* h, int B);
int ac_mimi_stream_decode_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream);
size_t ac_mimi_stream_decode_workspace_bytes(const ac_handle* h, int B, int F);
int ac_mimi_stream_decode(ac_handle* h, void* state_dev, size_t state_bytes, const int64_t* toks_dev, int B, int F, int K,
                          float* sig_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Independent sessions on one Mimi stream state: pushes of a SUBSET of its B streams ("slots").  The state is
 * prepared whole by ac_mimi_stream_reset / _decode_reset (that call writes the header and registers the address, for the capacity B);
 * a slot restarts alone through the same call with a reset mask, and the calls below run any of the slots while the others keep what
 * they hold.
 *   slots_host [n]  the slot list in host memory: 1 <= n <= B distinct values in [0, B).  The library reads it for every check, all
 *                   decided before anything is launched.
 *   slots_dev  [n]  the caller's device copy of the same list, which the kernels read (the library neither allocates nor copies).
 *                   Whatever it holds, the kernels index only inside the state: an entry outside [0, B) makes that row touch no state.
 * Row i of sig_dev [n, F * hop] / toks_dev [n, F, K] belongs to slot slots_host[i], each at its own position (conv caches, K/V rings
 * and the position go through the list; every activation stays dense).  Every buffer, scale and launch is that of a lockstep push of
 * B = n streams, so the workspace is ac_mimi_stream_workspace_bytes(h, n, F) / _decode_workspace_bytes(h, n, F), and the bits of a
 * slot's result are those of the lockstep stream of batch n fed the same rows: they depend neither on the slot's index, nor on the
 * order of the list, nor on what the other rows or the unlisted slots carry.  (The decode side picks the route of its linear layers
 * from the dense row count n * F * resample_stride, as ac_mimi_stream_decode does from B: "mstream_skinny" in ac_debug_set.)  Mimi
 * pads with zeros: fresh and warm slots share any call at any F >= 1, and the handle keeps no per-slot record.  A lockstep push on the
 * same state is the push of all B slots in order.
 * AC_EINVAL for a state never reset on this handle, reset as the other kind or for another B, n outside [1, B], a slot outside [0, B)
 * or listed twice, a null pointer, K or F out of range, a non-Mimi handle; AC_ENOMEM for a short state or workspace; AC_ESTATE for a
 * handle loaded without the half it needs.  After a refusal the handle and the state are as they were; nothing allocates or
 * synchronises. */
int ac_mimi_stream_encode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev,
                                int n, const float* sig_dev, int F, int K, int64_t* toks_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream);
int ac_mimi_stream_decode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev,
                                int n, const int64_t* toks_dev, int F, int K, float* sig_dev, void* workspace_dev,
                                size_t workspace_bytes, void* stream);

/* Streaming EnCodec encode and decode: the same contract as the Mimi calls above on an EnCodec handle -- B streams, F whole frames per
 * stream and push, tokens [B,F,K] and samples [B, F * hop] in ac_encode's / ac_decode's layouts; the caller owns the state
 * (ac_encodec_stream_state_bytes / _decode_state_bytes(h, B) bytes, 256-byte aligned) and the workspace (_workspace_bytes(h, B, F));
 * nothing allocates or synchronises.  Per stream the state holds the last k - stride input rows of every causal conv, the previous
 * input row of every transposed conv, h and c of both LSTM layers (zero after a reset), the frame count and a "fresh" flag
 * (DESIGN.md "Streaming EnCodec").  An encode state and a decode state have their own magic and layout and are registered separately.
 * EnCodec pads by reflection, so a fresh stream's conv history is the mirror image of its own first rows, and the FIRST push after a
 * reset must bring F >= max(kernel_size, last_kernel_size) frames (7: 93 ms; AC_EINVAL otherwise -- with fewer the reference itself
 * switches to its small-input padding rule and no stream could reproduce the one-shot result).  From then on any F >= 1; the tokens /
 * samples of a stream are those ac_encode / ac_decode give on its whole signal / token sequence (up to rounding: split16 scales are
 * taken per stream and push) and do not depend on the other streams.  The streams of a state reset together: reset_mask_dev must be
 * NULL (AC_EINVAL).  AC_EINVAL for a non-EnCodec handle (*_state_bytes and *_workspace_bytes return 0), a state this handle never
 * reset, reset for another B or reset as the other kind; AC_ENOMEM for a state or workspace that is too small; AC_ESTATE for a handle
 * loaded without the half it needs.  These are decided on the host before anything is launched: the handle and the state stay as
 * they were. */
size_t ac_encodec_stream_state_bytes(const ac_handle* h, int B);
int ac_encodec_stream_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream);
size_t ac_encodec_stream_workspace_bytes(const ac_handle* h, int B, int F);
int ac_encodec_stream_encode(ac_handle* h, void* state_dev, size_t state_bytes, const float* sig_dev, int B, int F, int K,
                             int64_t* toks_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
size_t ac_encodec_stream_decode_state_bytes(const ac_handle* h, int B);
int ac_encodec_stream_decode_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, const uint8_t* reset_mask_dev, void* stream);
size_t ac_encodec_stream_decode_workspace_bytes(const ac_handle* h, int B, int F);
int ac_encodec_stream_decode(ac_handle* h, void* state_dev, size_t state_bytes, const int64_t* toks_dev, int B, int F, int K,
                             float* sig_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Independent sessions on one EnCodec stream state: pushes and resets of a SUBSET of its B streams ("slots").
 * A state is prepared once, whole, by ac_encodec_stream_reset / _decode_reset (that call writes the header and registers the address);
 * from then on the calls below restart and run any of its slots while the others keep what they hold.
 *   slots_host [n]  the slot list in host memory: 1 <= n <= B distinct values in [0, B).  The library reads it for every check, all
 *                   decided before anything is launched.
 *   slots_dev  [n]  the caller's device copy of the same list, which the kernels read (the library neither allocates nor copies).
 *                   Whatever it holds, the kernels index only inside the state: an entry outside [0, B) makes that row touch no state.
 * ac_encodec_stream_reset_slots / _decode_reset_slots: the listed slots start afresh (frame count 0, fresh, LSTM h = c = 0) in one
 * launch; no other byte of the state changes.
 * ac_encodec_stream_encode_slots / _decode_slots: one push of F whole frames for the n listed slots.  Row i of sig_dev [n, F * hop] /
 * toks_dev [n, F, K] belongs to slot slots_host[i]; every buffer, scale and launch is that of a lockstep push of B = n streams, so the
 * workspace is ac_encodec_stream_workspace_bytes(h, n, F) / _decode_workspace_bytes(h, n, F), and the bits of a slot's result are those
 * of the lockstep stream fed the same rows: they depend neither on the slot's index, nor on the order of the list, nor on what the other
 * rows or the unlisted slots carry.  The handle keeps a freshness flag per slot: if ANY listed slot is fresh (no push since its reset),
 * F >= max(kernel_size, last_kernel_size) (7), AC_EINVAL otherwise; fresh and warm slots may share a call when F allows.  A lockstep
 * push (ac_encodec_stream_encode / _decode) on the same state is the push of all B slots in order, and needs the warm-up F while any
 * slot is fresh.
 * AC_EINVAL for a state never reset whole on this handle, reset as the other kind or for another B, n outside [1, B], a slot outside
 * [0, B) or listed twice, a null pointer, K out of range, a non-EnCodec handle; AC_ENOMEM for a short state or workspace; AC_ESTATE
 * for a handle loaded without the half it needs.  After a refusal the handle and the state are as they were. */
int ac_encodec_stream_reset_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev,
                                  int n, void* stream);
int ac_encodec_stream_decode_reset_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host,
                                         const int* slots_dev, int n, void* stream);
int ac_encodec_stream_encode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev,
                                   int n, const float* sig_dev, int F, int K, int64_t* toks_dev, void* workspace_dev,
                                   size_t workspace_bytes, void* stream);
int ac_encodec_stream_decode_slots(ac_handle* h, void* state_dev, size_t state_bytes, int B, const int* slots_host, const int* slots_dev,
                                   int n, const int64_t* toks_dev, int F, int K, float* sig_dev, void* workspace_dev,
                                   size_t workspace_bytes, void* stream);

/* Copy the first K codebooks to embs_dev [K, codebook_size, ac_codebook_dim] fp32 (encodec.py:74-79;
 * mimi.py:52-62 `latent=True`). */
int ac_embs(ac_handle* h, int K, float* embs_dev, void* stream);
/* Mimi `latent=False` (mimi.py:63-90): every code vector through its quantiser's output projection
 * -> embs_dev [K, codebook_size, hidden].  AC_EINVAL on EnCodec handles. */
int ac_embs_projected(ac_handle* h, int K, float* embs_dev, void* stream);

/* Sample-rate conversion at the Codec boundary (audiocodecs/codec.py:59-63,95-99 call
 * torchaudio.functional.resample): polyphase windowed-sinc FIR.  kern_dev [n][taps] is the filter
 * bank (n = new_rate/gcd phases, stride o = orig_rate/gcd, `width` zero samples of left padding);
 * y[b][i*n + ph] = sum_k kern[ph][k] * x[b][i*o + k - width], L_out = ceil(n*L/o).  Handle-free. */
int ac_resample(const float* x_dev, int B, int L, const float* kern_dev, int n, int o, int taps, int width,
                float* y_dev, int L_out, void* stream);

/* The same conversion push by push, for streams: B streams share one rate pair and one phase; each push brings L
 * samples per stream and returns the outputs that no later input can change.  With taps = 2 * width + o, output group i (outputs
 * i*n .. i*n + n - 1) reads the inputs i*o - width .. i*o - width + taps - 1 and is complete once width + o + i*o samples are in: after
 * `total` samples G(total) = total < width + o ? 0 : (total - width - o) / o + 1 groups are.  A push emits the groups
 * G(consumed) .. G(consumed + L) - 1, i.e. n * (G(after) - G(before)) samples -- possibly none, and not the same number every push.  A
 * push with finish != 0 takes all later input as zero and emits the rest, up to ceil(n * total / o) outputs in all: ac_resample's
 * length, and, concatenated, ac_resample's values bit for bit (the same fp32 chain per output, ascending taps).  The added latency is
 * width + o - 1 input samples (0.5 ms for 16 <-> 24 kHz).
 *
 * Handle-free.  The caller owns the state: ac_resample_stream_state_bytes(B, taps) bytes of device memory, 256-byte aligned, holding a
 * header (a magic of its own, B, n, o, taps, width), the samples consumed per stream and the last taps - 1 input samples per stream
 * (zeros on a fresh stream).  The caller also keeps the count of samples consumed since the reset and passes it to every push
 * (ac_resample_stream_out_len needs it to size the output before the launch); the device compares it, and the geometry, with the state
 * and writes NaN instead of samples when they disagree (a state never reset, reset for another geometry, pushed after its finish, or a
 * count that is not the state's).  ac_resample_stream_out_len is pure host arithmetic: the number of samples per stream a push of L
 * samples (or that push as the closing one) emits; AC_EINVAL (-1) for a negative or overflowing argument.
 * ac_resample_stream_push reads x_dev [B] rows of L samples x_pitch floats apart and writes y_dev [B] rows y_pitch floats apart, of
 * which y_capacity floats per row are the caller's to write: with the pitch a caller can have the samples written straight behind
 * those it already holds.  AC_EINVAL for a null or misaligned state, geometry that is not a filter bank's (taps != 2 * width + o,
 * taps > 8192, B, n, o < 1), a negative L or count, or a pitch shorter than its row; AC_ENOMEM for a state shorter than
 * ac_resample_stream_state_bytes or y_capacity below the push's output length: all decided on the host before anything is launched,
 * and the state stays as it was.  A push is two launches on the caller's stream (one when it emits nothing, none for L == 0 without
 * finish); nothing allocates or synchronises.  After the closing push only a reset makes the state usable again. */
long long ac_resample_stream_out_len(long long consumed, int L, int n, int o, int width, int finish);
size_t ac_resample_stream_state_bytes(int B, int taps);
int ac_resample_stream_reset(void* state_dev, size_t state_bytes, int B, int n, int o, int taps, int width, void* stream);
int ac_resample_stream_push(void* state_dev, size_t state_bytes, const float* x_dev, long long x_pitch, int B, int L, long long consumed,
                            const float* kern_dev, int n, int o, int taps, int width, float* y_dev, long long y_pitch, long long y_capacity,
                            int finish, void* stream);

/* Independent sessions on one resampler state: pushes and resets of a SUBSET of its B streams ("slots"), each at its own phase
 * (DESIGN.md section 8h).  The state is the one above, prepared whole by ac_resample_stream_reset (that call alone writes the header),
 * and serves both forms.
 *   slots_host [n_rows], consumed_host [n_rows]  the slot list (1 <= n_rows <= B distinct values in [0, B)) and, per listed slot, the
 *                   caller's count of the samples it has consumed, in host memory.  The library reads them for every check and to size
 *                   the grid, all decided before anything is launched.
 *   slots_dev [n_rows], consumed_dev [n_rows]    the caller's device copies, which the kernels read (the library neither allocates nor
 *                   copies; both may lie in one buffer, so that one host-to-device copy brings them).  Whatever they hold, the kernels
 *                   index only inside the state and the first max_r m_r floats of a y row: a row whose slot is outside [0, B), or whose
 *                   count is negative or not the state's, gets NaN outputs and touches no state.
 * ac_resample_stream_reset_slots: the listed slots start afresh (count 0, zero history) in one launch; no other byte of the state
 * changes, and nothing at all when the header is not that of the arguments.
 * ac_resample_stream_push_slots: row r of x_dev brings L samples to slot slots_host[r] and emits
 * m_r = ac_resample_stream_out_len(consumed_host[r], L, n, o, width, finish) samples into y_dev[r][0 .. m_r); m_r differs between the rows
 * of one call, and what lies behind m_r in a row is left untouched.  L and finish hold for every row of the call.  Per output the fp32
 * chain is ac_resample_stream_push's, so a slot's pushes and its closing push, concatenated, are ac_resample of its whole signal bit for
 * bit, whichever slot it sits in, whatever the other rows carry and however many calls it sits out.  Two launches (one when no row emits,
 * none for L == 0 without finish).
 * AC_EINVAL for a null or misaligned state, geometry that is not a filter bank's, n_rows outside [1, B], a slot outside [0, B) or listed
 * twice, a negative or overflowing count, a negative L, a null list, or a pitch shorter than its row (y_pitch: than the longest m_r);
 * AC_ENOMEM for a short state or y_capacity below the longest m_r.  After a refusal the state is as it was; nothing allocates or
 * synchronises. */
int ac_resample_stream_reset_slots(void* state_dev, size_t state_bytes, int B, int n, int o, int taps, int width, const int* slots_host,
                                   const int* slots_dev, int n_rows, void* stream);
int ac_resample_stream_push_slots(void* state_dev, size_t state_bytes, int B, const int* slots_host, const long long* consumed_host,
                                  const int* slots_dev, const long long* consumed_dev, int n_rows, const float* x_dev, long long x_pitch,
                                  int L, const float* kern_dev, int n, int o, int taps, int width, float* y_dev, long long y_pitch,
                                  long long y_capacity, int finish, void* stream);

/* Cosine k-nearest-neighbour feature matching: for each of Q query rows [H] the k = min(topk, valid rows) rows of
 * a matching set [M][H] with the largest cosine similarity, and the mean of those rows -- the single-codebook voice-conversion step of
 * downstream/test_vc.py:116-128 (`knn(...).mean(dim=-2)`) without its [Q][M] distance matrix, its top-k and its gather.  Both sides are
 * L2-normalised first and the similarity is ONE dot product of unit vectors in split16 arithmetic (the error of an fp32 FMA chain).
 * Neighbours are ordered by (similarity descending, index ascending): equal computed similarities go to the lower index.
 * Handle-free; the caller owns every buffer; all fp32 buffers and the packed image are 16-byte aligned; H is one of 32, 64, 128, 256,
 * 512 (zero-pad a narrower width: zeros leave the cosine alone); 1 <= topk <= 8; 1 <= M, Q <= 2^24 rows.
 *   ac_knn_packed_bytes(M, H)      bytes of the packed image of a set (0 for arguments ac_knn_pack refuses).
 *   ac_knn_pack                    one launch: normalises the rows and writes the image and a validity word per row.  A row whose largest
 *                                  magnitude is zero or denormal, or that holds an inf or a NaN, is invalid and is never matched.  Pack
 *                                  once per matching set and match any number of query batches against it.
 *   ac_knn_num_splits(Q, M, H, n)  the number of slices of the set a match walks side by side: n itself for 1 <= n <= 64, the library's
 *                                  choice from (Q, M, H) for n = 0 (few queries against a long set: up to 16; 1 from 1024 query waves on and
 *                                  for sets of at most 240 rows).  Pure host arithmetic; AC_EINVAL for arguments out of range.  Every split count
 *                                  returns the same indices, similarities and output, bit for bit.
 *   ac_knn_workspace_bytes         bytes of workspace a match with these arguments needs (0 for arguments it refuses).
 *   ac_knn_match                   two launches on `stream`.  set_dev is the ORIGINAL fp32 set (the rows that are averaged), packed_dev its
 *                                  image for the same (M, H).  Any of the results may be NULL:
 *                                    out_dev [Q][H]     the mean of the k nearest rows: summed nearest first in fp32, times 1 / k
 *                                    idx_dev [Q][topk]  their indices, nearest first, -1 behind k
 *                                    sim_dev [Q][topk]  their cosine similarities, NaN behind k
 *                                  A query row that is invalid in the sense above gets a NaN output row, indices -1 and NaN similarities and
 *                                  disturbs no other row.
 * AC_EINVAL for a null or misaligned pointer, a width, topk, row count or split count out of range; AC_ENOMEM for a packed buffer or a
 * workspace that is too short; all decided on the host before anything is launched.  Nothing allocates or synchronises. */
size_t ac_knn_packed_bytes(long long M, int H);
int ac_knn_pack(const float* set_dev, long long M, int H, void* packed_dev, size_t packed_bytes, void* stream);
int ac_knn_num_splits(long long Q, long long M, int H, int num_splits);
size_t ac_knn_workspace_bytes(long long Q, long long M, int H, int topk, int num_splits);
int ac_knn_match(const float* query_dev, long long Q, const float* set_dev, const void* packed_dev, long long M, int H, int topk,
                 int num_splits, float* out_dev, int64_t* idx_dev, float* sim_dev, void* workspace_dev, size_t workspace_bytes,
                 void* stream);

/* Fused STFT and mel spectral distances: the two resynthesis metrics of the reference's evaluation recipes
 * (downstream/metrics/stft_distance.py:49-69, mel_distance.py:57-61) at their defaults -- signals at 16 kHz, n_fft = win_length = 1024,
 * hop 320, periodic Hann window, center = True with reflect padding, 513 bins, 80 HTK mel filters over 0 .. 8000 Hz without norm,
 * dB = 10 log10(max(x, 1e-10)) -- for P hypotheses of B clips against one reference, F = 1 + L / 320 frames a clip:
 *     stft[p][b] = mean over frames of sqrt(sum over the 513 bins of (dB |X_hyp| - dB |X_ref|)^2),   mel[p][b] likewise over the 80 mels.
 * One split16 MFMA GEMM per tile of 16 frames with the epilogue in registers: no spectrogram reaches memory, the workspace holds one
 * fp32 per (hypothesis, clip, frame) and metric.  A clip's results do not depend on P, on B or on the other clips of the call; swapping
 * hypothesis and reference returns the same bits; equal signals give exactly 0; a clip that holds an inf or a NaN gets NaN scores and
 * disturbs no other clip.  Handle-free; the caller owns every buffer; the source, the tables and the workspace are 16-byte aligned, signals
 * and results 4-byte (a row of a larger batch serves as it stands); 1 <= P <= 4, 1 <= B,
 * 512 < L <= 2^24 (and P B ceil(F / 16) < 2^31).
 *   ac_specdist_source_count()     doubles of the tables' fp64 source: cos(2 pi j / 1024) [1024], then the filterbank [513][80].
 *   ac_specdist_source             fills that source in HOST memory (pure host arithmetic in fp64, angles reduced as integers; no GPU).
 *   ac_specdist_tables_bytes()     bytes of the device tables (the windowed DFT basis and the filterbank as split16 fp16 planes).
 *   ac_specdist_tables             one launch: builds the tables from the caller's DEVICE copy of the source.  Build once per device.
 *   ac_specdist_num_frames(L)      F (0 for an L that ac_specdist refuses).
 *   ac_specdist_workspace_bytes    bytes of workspace a call with these arguments needs (0 for arguments it refuses).
 *   ac_specdist                    two launches on `stream`.  hyp_dev [P][B][L], ref_dev [B][L], stft_out / mel_out [P][B];
 *                                  stft_frames_out / mel_frames_out [P][B][F] (the per-frame distances) may be NULL.
 * AC_EINVAL for a null or misaligned pointer, a count out of range or L <= 512; AC_ENOMEM for a table buffer or a workspace that is too
 * short; all decided on the host before anything is launched.  Nothing allocates or synchronises. */
size_t ac_specdist_source_count(void);
int ac_specdist_source(double* src_host, size_t count);
size_t ac_specdist_tables_bytes(void);
int ac_specdist_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream);
long long ac_specdist_num_frames(long long L);
size_t ac_specdist_workspace_bytes(int P, long long B, long long L);
int ac_specdist(const float* hyp_dev, const float* ref_dev, int P, long long B, long long L, const void* tables_dev, float* stft_out,
                float* mel_out, float* stft_frames_out, float* mel_frames_out, void* workspace_dev, size_t workspace_bytes, void* stream);

/* STOI of P hypotheses of B clips against one reference: downstream/metrics/stoi.py behind its resampling to
 * 16 kHz -- pystoi's algorithm at its defaults (extended = False), restated: 16 -> 10 kHz by a Kaiser-windowed polyphase FIR (581 taps, up 5,
 * down 8), removal of the frames of 256 at hop 128 that lie more than 40 dB below the loudest frame of the REFERENCE, overlap-add of the
 * kept frames of both signals, 512-point STFT, 15 third-octave band envelopes, the clipped and normalised correlation over sliding
 * segments of 30 frames.  All signals are fp32 at 16 kHz with L16 samples, ceil(5 L16 / 8) >= 256 and L16 <= 2^24;
 * F0 = (ceil(5 L16 / 8) - 256) / 128 + 1 frames exist before the removal; 1 <= P <= 4.  The score of a pair with fewer than 30 STFT frames
 * left is 1e-5; a clip with an inf or a NaN in either signal gets NaN.  A clip's values depend on nothing else in the call.
 *   ac_stoi_source_count()      doubles of the tables' fp64 source: hanning(258)[1:-1] [256], cos(2 pi j / 512) [512], the FIR h [581].
 *   ac_stoi_source              fills that source in HOST memory (pure host arithmetic in fp64; no GPU).
 *   ac_stoi_tables_bytes()      bytes of the device tables (window and FIR bank in fp32, the windowed DFT basis as split16 fp16 planes).
 *   ac_stoi_tables              one launch: builds the tables from the caller's DEVICE copy of the source.  Build once per device.
 *   ac_stoi_num_frames(L16)     F0 (0 for an L16 that ac_stoi refuses).
 *   ac_stoi_workspace_bytes     bytes of workspace a call with these arguments needs (0 for arguments it refuses).
 *   ac_stoi                     six launches on `stream`, none sized by anything the device computes.  hyp_dev [P][B][L16],
 *                               ref_dev [B][L16], score_out [P][B].  Optional (may be NULL): kept_out [B][F0] bytes 0 / 1, the frames
 *                               kept; num_segments_out [B], S = max(K - 30, 0) for K kept frames; segments_out [P][B][max(F0 - 30, 0)],
 *                               per segment the sum of the 15 band correlations / 15, NaN past S.
 * AC_EINVAL for a null or misaligned pointer, a count out of range or a length out of range; AC_ENOMEM for a table buffer or a
 * workspace that is too short; all decided on the host before anything is launched.  Nothing allocates or synchronises. */
size_t ac_stoi_source_count(void);
int ac_stoi_source(double* src_host, size_t count);
size_t ac_stoi_tables_bytes(void);
int ac_stoi_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream);
long long ac_stoi_num_frames(long long L16);
size_t ac_stoi_workspace_bytes(int P, long long B, long long L16);
int ac_stoi(const float* hyp_dev, const float* ref_dev, int P, long long B, long long L16, const void* tables_dev, float* score_out,
            uint8_t* kept_out, int32_t* num_segments_out, float* segments_out, void* workspace_dev, size_t workspace_bytes, void* stream);

/* The DNSMOS P.808 score of a batch of clips at 16 kHz (handle-free): librosa's log-mel front end at the defaults
 * the reference calls it with (n_fft 321, hop 160, periodic Hann, center = True with zero padding, power 2, 120 Slaney mel filters over
 * 0 .. 8000 Hz with Slaney norm, (power_to_db(S, ref = max) + 40) / 40) per window of 900 frames, then the fixed P.808 net: five 3 x 3
 * convolutions (1 -> 32 -> 32 -> 32 -> 32 -> 64, ReLU, 2 x 2 max pools behind the first, second and fourth), the global maximum and three
 * dense layers.  The convolutions with 32 input channels run on the fp16 matrix pipe in split16 arithmetic; a window's values depend on
 * nothing else in the call.
 *   ac_dnsmos_source_count()     doubles of the front end's fp64 source: cos(2 pi j / 321) [321], sin [321], the filterbank [161][120].
 *   ac_dnsmos_source             fills that source in HOST memory (pure host arithmetic in fp64; no GPU).
 *   ac_dnsmos_tables_bytes()     bytes of the device tables (the windowed DFT basis as split16 fp16 planes, the filterbank in fp32).
 *   ac_dnsmos_tables             one launch: builds the tables from the caller's DEVICE copy of the source.  Build once per device.
 *   ac_dnsmos_weights_count()    floats of the net's weights as one flat fp32 array, in this order: conv5.w [32][1][3][3], conv5.b [32],
 *                                conv6.w [32][32][3][3], conv6.b, conv7.w, conv7.b, conv8.w, conv8.b, conv9.w [64][32][3][3], conv9.b [64],
 *                                dense3.w [64 in][64 out], dense3.b, dense4.w, dense4.b, dense5.w [64][1], dense5.b [1].
 *   ac_dnsmos_packed_bytes()     bytes of the packed image of those weights.
 *   ac_dnsmos_pack               one launch: packs the caller's DEVICE copy of the flat weights (fragment images of the matrix pipe, one
 *                                power-of-two scale per output channel).  Pack once per device.
 *   ac_dnsmos_workspace_bytes    bytes of workspace for S windows of H x W features (0 for arguments refused).  Windows are walked in
 *                                chunks, so the bound does not grow with S beyond one chunk (32 windows at 900 x 120) plus 4 S bytes.
 *   ac_dnsmos_net                the net alone: feats_dev [S][H][W] (H = time, W = mel; H, W >= 8, run-time values) -> score_out [S].
 *                                Optional (may be NULL): the four stored feature maps, channels last, layer1_out [S][H/2][W/2][32],
 *                                layer2_out and layer3_out [S][H/4][W/4][32], layer4_out [S][H/8][W/8][32], and vec_out [S][64], the global
 *                                maxima.  Seven launches per chunk, none of them a memset node.
 *   ac_dnsmos                    the whole call: sig_dev [B][L16]; plan_dev, int32: [S][4] = (clip, first sample, clip length, index among
 *                                the clip's windows) of every window, the windows of a clip together and the clips in order, then
 *                                [B][2] = (first window, number of windows >= 1) of every clip.  Sample j of a window is sample
 *                                (first + j) mod length of its clip -- the reference doubles a short clip until it holds 9.01 s.  The host
 *                                decides which windows exist (audiocodecs_amd.dnsmos.dnsmos_segments).  score_out [B], the mean over a
 *                                clip's windows; optional segments_out [B][Smax] (NaN behind a clip's count) and feats_out [S][900][120].
 *                                A window with an inf or a NaN among its samples scores NaN.  Eight launches per chunk and one at the end.
 * AC_EINVAL for a null or misaligned pointer or a count out of range; AC_ENOMEM for a buffer or a workspace that is too short; all decided
 * on the host before anything is launched.  Nothing allocates or synchronises.  The plan is read on the device only: entries out of range
 * are clamped there, so no read leaves the signals. */
size_t ac_dnsmos_source_count(void);
int ac_dnsmos_source(double* src_host, size_t count);
size_t ac_dnsmos_tables_bytes(void);
int ac_dnsmos_tables(const double* src_dev, void* tables_dev, size_t tables_bytes, void* stream);
size_t ac_dnsmos_weights_count(void);
size_t ac_dnsmos_packed_bytes(void);
int ac_dnsmos_pack(const float* weights_dev, size_t count, void* packed_dev, size_t packed_bytes, void* stream);
size_t ac_dnsmos_workspace_bytes(long long S, int H, int W);
int ac_dnsmos_net(const float* feats_dev, long long S, int H, int W, const void* packed_dev, float* score_out, float* layer1_out, float* layer2_out,
                  float* layer3_out, float* layer4_out, float* vec_out, void* workspace_dev, size_t workspace_bytes, void* stream);
int ac_dnsmos(const float* sig_dev, long long B, long long L16, const int32_t* plan_dev, long long S, int Smax, const void* tables_dev,
              const void* packed_dev, float* score_out, float* segments_out, float* feats_out, void* workspace_dev, size_t workspace_bytes,
              void* stream);

/* Token histogram and codebook utilisation (handle-free): downstream/metrics/codebook_util.py without its B == 1,
 * its unique() per codebook and its 2 K host copies per clip.  The caller owns the state, ONE 8-byte aligned device buffer of int64 words,
 *     counts [K][C], total, bad:   counts[k][c] the times id c was seen in codebook k, total the frames counted, bad the ids outside
 *     [0, C) among the counted frames (they are not counted in `counts`, never index anything and never fault),
 * and zeroes it before the first call; calls accumulate.  1 <= K <= 64, 2 <= C <= 2^20, B N K <= 2^40.  Counts are exact integers.
 *   ac_tokstats_state_bytes(K, C)  bytes of the state, (K C + 2) * 8 (0 for a K or a C out of range).
 *   ac_tokstats_form(K, C)         which of the two forms a call takes, a pure function of (K, C): G >= 1, the tiled form -- a workgroup keeps
 *                                  the histogram of G = min(K, 16384 / C) codebooks in LDS and flushes its non-zero bins with 64-bit atomic
 *                                  adds; with G < K the groups of codebooks are a grid dimension -- or 0, the direct form for C > 16384: one
 *                                  64-bit global atomic add per token.  AC_EINVAL for a K or a C out of range.
 *   ac_tokstats_accumulate         one launch on `stream`: one pass over toks_dev [B][N][K] (int64, contiguous, K fastest).  nvalid_dev [B]
 *                                  (int32) may be NULL: every frame of every clip; otherwise the frames n >= nvalid[b] of clip b are skipped.
 *                                  B == 0 or N == 0 launches nothing and returns 0.
 *   ac_tokstats_summary            one launch, one workgroup per codebook: out_dev [K][4] doubles = (valid, entropy, util, norm_entropy) --
 *                                  valid the non-zero bins, entropy = -sum p log2 p over p = counts / total > 0, util = valid / C and
 *                                  norm_entropy = entropy / log2(valid) where valid > 1, else both 0 (codebook_util.py:54-70, in fp64 and in a
 *                                  fixed order).  total == 0 gives zeros, never a NaN.
 * AC_EINVAL for a null or misaligned pointer or a count out of range; AC_ENOMEM for a state that is too short; all decided on the host
 * before anything is launched.  Nothing allocates, synchronises or is read back, and no launch is sized by what the device computed: both
 * calls can be captured into a graph. */
size_t ac_tokstats_state_bytes(int K, int C);
int ac_tokstats_form(int K, int C);
int ac_tokstats_accumulate(const int64_t* toks_dev, long long B, long long N, int K, int C, const int32_t* nvalid_dev, void* state_dev,
                           size_t state_bytes, void* stream);
int ac_tokstats_summary(const void* state_dev, int K, int C, double* out_dev, void* stream);

/* Fused token sampling and masked token resampling (handle-free): the reference's chain of softmax, top-k or top-p,
 * multinomial and gather (codec.py:121-180, downstream/models/llama3.py:944-996) for R rows of C logits in ONE launch, each row's draw
 * addressed by a counter of the repository's PRNG (audiocodecs_amd/prng.py) so that a result can be checked token by token.
 *   ac_sample_form(C)   1: one wave per row (C <= 1024); 2: one workgroup of ceil(C / 1024) waves per row.  A pure function of C;
 *                       AC_EINVAL outside 2 <= C <= 16384.
 *   ac_sample_tokens    row r reads C fp32 logits at logits_dev + (row_index_dev ? row_index_dev[r] : r) * row_stride (the caller keeps
 *                       the indices inside the table) and writes one int64 to out_dev[r]:
 *       weights   w_i = exp((l_i - max_j l_j) / temp), temp > 0; -inf has weight 0 and is never returned.  A row that holds a NaN or whose
 *                 maximum is not finite returns -1.
 *       kept set  entries ranked by value descending, ties by ascending index (decided on the bits of the logits; -0 equals +0).
 *                 top_k = k > 0 keeps the ranks < k; top_p = p >= 0 keeps rank j iff (the weight of the ranks < j) / (the weight of all)
 *                 <= p, and p = 1 keeps everything; neither (top_k = 0, top_p < 0) keeps everything; both are refused.
 *       draw      t = u * (the weight of the kept set); the result is the first kept index, in ascending index order, whose inclusive
 *                 prefix sum of the kept weights exceeds t.  The sums are fp32: a result may differ from the exact statement where u
 *                 lies within their rounding of an interval's end or a top-p cut lies within it of p (section 8o bounds both by 2^-18).
 *                 Whatever the rounding, the result has a positive weight and lies in the kept set.
 *       words     word i of the stream is mix(key + (i + 1) * 0x9E3779B97F4A7C15) (prng.py); row r uses the words 2 (offset + r), the
 *                 mask word, and 2 (offset + r) + 1, the draw word, as u = (word >> 40) * 2^-24.  offset_dev [1] (int64), when given, is
 *                 read by the kernel and added to `offset`: a captured graph advances the stream between replays.
 *       mask      mask_p >= 0: row r is sampled iff u_mask < mask_p (fp32); otherwise out_dev[r] = fallback_dev[r] and the row is not read.
 *                 mask_p < 0: every row is sampled and fallback_dev is not used.
 * AC_EINVAL, decided on the host before the launch: a null logits_dev or out_dev; a pointer that is not aligned to its element; R < 0 or
 * R >= 2^31; C outside 2..16384; row_stride < C; temp not finite, <= 0 or so small that 1 / temp is not finite; top_k < 0 or > C;
 * top_p > 1 or NaN; both cuts; mask_p > 1 or NaN; mask_p >= 0 without fallback_dev.  R == 0 launches nothing.  No workspace; nothing
 * allocates, synchronises or is read back: the call can be captured into a graph. */
int ac_sample_form(int C);
int ac_sample_tokens(const float* logits_dev, long long row_stride, const int64_t* row_index_dev, long long R, int C, float temp, int top_k,
                     float top_p, uint64_t key, uint64_t offset, const int64_t* offset_dev, float mask_p, const int64_t* fallback_dev,
                     int64_t* out_dev, void* stream);

/* WavLM x-vector speaker embeddings: inference of transformers' WavLMForXVector for the microsoft/wavlm-base-sv
 * family on one more ac_handle kind -- 7-layer conv front end (GroupNorm over time behind the first), feature projection, grouped
 * positional conv, post-LN transformer layers with gated relative-position bias and key padding, weighted layer sum, projector, TDNN
 * layers, statistic pooling, feature_extractor.  Weights go in through ac_load_weights under their WavLMForXVector state-dict names
 * (classifier.* and objective.* are accepted and unused; the positional conv's weight norm -- over dims (0, 1), one norm per tap --
 * is folded on the host at ac_finalize unless wavlm.encoder.pos_conv_embed.conv.weight itself is loaded) plus "spk.bucket_table", the
 * relative-position buckets of the offsets
 * -2 max_distance .. 2 max_distance as floats (2 * 2 * max_distance + 1 values, built by the caller with the backend's own fp32
 * operations: the table is data).
 *   ac_spk_create          AC_EINVAL for anything but feat_extract_norm "group", no conv bias, post-LN layers, the weighted layer sum, no
 *                          adapter, head dim 64, conv kernels (10,3,3,3,3,2,2) with strides (5,2,2,2,2,2,2), and widths the kernels take
 *                          (conv_dim % 32, hidden % 64, per-group width of the positional conv % 16, TDNN kernels summing to
 *                          receptive field 15); decided before a device is looked for.
 *   ac_spk_num_frames(L)   (L - 400) / 320 + 1 frames of a clip of L samples at 16 kHz (0 below 400 samples); handle-free.
 *   ac_spk_workspace_bytes workspace of one ac_spk_embed call: the batch is walked in chunks of max_chunk_clips clips (0: as many as keep
 *                          the workspace under 1 GiB, at least one), so the size stops growing with B.
 *   ac_spk_embed           sig16k_dev [B][L] fp32 at 16 kHz, raw (no normalisation).  valid_dev [B] int32 or NULL: the samples of clip b
 *                          that are speech; frames t >= Lf = (valid - 400) / 320 + 1 are zeroed behind the feature projection and masked as
 *                          attention keys, and the rows [0, min(Lf - 8, T - 14)) are pooled (NULL: all T - 14).  The lengths are read on
 *                          the device: the call copies nothing back.  A clip with one pooled row has a NaN embedding (unbiased std of one
 *                          row, as in the backend); with none, also NaN.  L < 4880 (T < 15: no pooled row at all) is AC_EINVAL.
 *                          emb_out [B][xvector_dim].  stages: optional outputs, each pointer may be NULL.
 *   ac_spk_cosine          out[b] = <a_b, b_b> / (max(|a_b|, eps) max(|b_b|, eps)), eps 1e-8 (torch.nn.functional.cosine_similarity), one
 *                          wave per pair; handle-free.
 * Results of a clip do not depend on the clips beside it or on the chunking. */
typedef struct ac_spk_config {
    int32_t struct_size;
    int32_t conv_dim;                       /* width of all conv layers (512)                      */
    int32_t num_conv_layers;                /* 7                                                   */
    int32_t conv_kernel[AC_MAX_RATIOS];     /* (10,3,3,3,3,2,2)                                    */
    int32_t conv_stride[AC_MAX_RATIOS];     /* (5,2,2,2,2,2,2)                                     */
    int32_t hidden_size;                    /* 768                                                 */
    int32_t num_hidden_layers;              /* 12                                                  */
    int32_t num_attention_heads;            /* 12                                                  */
    int32_t intermediate_size;              /* 3072                                                */
    int32_t num_conv_pos_embeddings;        /* 128                                                 */
    int32_t num_conv_pos_embedding_groups;  /* 16                                                  */
    int32_t num_buckets;                    /* 320                                                 */
    int32_t max_bucket_distance;            /* 800                                                 */
    int32_t num_tdnn_layers;                /* 5                                                   */
    int32_t tdnn_dim[AC_MAX_RATIOS];        /* (512,512,512,512,1500)                              */
    int32_t tdnn_kernel[AC_MAX_RATIOS];     /* (5,3,3,1,1)                                         */
    int32_t tdnn_dilation[AC_MAX_RATIOS];   /* (1,2,3,1,1)                                         */
    int32_t xvector_output_dim;             /* 512                                                 */
    int32_t feat_extract_norm_group;        /* 1: "group" (the only variant)                       */
    int32_t conv_bias;                      /* 0                                                   */
    int32_t do_stable_layer_norm;           /* 0                                                   */
    int32_t use_weighted_layer_sum;         /* 1                                                   */
    int32_t add_adapter;                    /* 0                                                   */
    int32_t max_chunk_clips;                /* clips per pass over the stack; 0: from the 1 GiB cap */
    int32_t device;
    float layer_norm_eps;                   /* 1e-5                                                */
} ac_spk_config;
typedef struct ac_spk_stages {
    float* feat;      /* [B][T][conv_dim]                 output of the last conv layer                                    */
    float* hidden;    /* [layers + 1][B][T][hidden]       the input of every layer, then the last layer's output           */
    float* tdnn;      /* [B][T - 14][tdnn_dim[last]]      output of the last TDNN layer                                    */
    float* pooled;    /* [B][2 * tdnn_dim[last]]          mean | unbiased std over the clip's pooled rows                  */
} ac_spk_stages;
int ac_spk_create(const ac_spk_config* cfg, ac_handle** out);
int ac_spk_num_frames(long long L);
size_t ac_spk_workspace_bytes(const ac_handle* h, int B, long long L);
int ac_spk_embed(ac_handle* h, const float* sig_dev, const int32_t* valid_dev, int B, long long L, float* emb_out, const ac_spk_stages* stages,
                 void* ws, size_t ws_bytes, void* stream);
int ac_spk_cosine(const float* a_dev, const float* b_dev, int B, int D, float* out_dev, void* stream);

/* The Llama decoder with a KV cache: inference of the downstream recipes' LlamaDecoder (RMSNorm, grouped-query
 * attention with rotary embeddings on interleaved pairs, SwiGLU feed-forward, one output head per codebook) and its token generation
 * loop on one more ac_handle kind.  fp32 weights, fp32 FMAs.  Weights go in through ac_load_weights under the model's state-dict names
 * (tok_embeddings.weight, layers.N.attention.{wq,wk,wv,wo}.weight, layers.N.attention_norm.weight, layers.N.feed_forward.{w1,w2,w3}.weight,
 * layers.N.ffn_norm.weight, norm.weight, output.weight or output.K.weight, prompt.weight) plus "lm.rope_cos" and "lm.rope_sin"
 * [2 * max_seq_len][head_dim / 2]: cos and sin of the rotary angles, built by the caller with the model's own fp32 operations (the
 * table is data; no kernel recomputes an angle).
 *   A STATE is a caller-owned, 256-byte aligned device buffer of ac_lm_state_bytes(B, capacity, max_steps) bytes: 64 header words
 *   (position, step counter, overflow flag, draw offset), alive / lens per row, the sampler's tokens, the pending logits [B][vocab] of
 *   the last row, hyp [B][max_steps] int64 and per layer the K and V planes [B][capacity][n_kv_heads][head_dim] (ac_lm_state_layout
 *   gives the byte offsets).  The position lives on the device; no call reads it back.
 *   ac_lm_create           AC_EINVAL unless dim % n_heads == 0, n_heads % n_kv_heads == 0 with 1, 2, 4 or 8 query heads per key/value
 *                          head, an even head dim <= 256, dim, ffn_dim and prompt_dim multiples of 4, 2 <= vocab_size <= 16384 (the
 *                          sampler's range); decided before a device is looked for.  prompt_dim 0: no prompt projection.
 *   ac_lm_reset            position 0, step 0, every row alive, the draw offset `offset`; B <= 64 rows, capacity <= 2 * max_seq_len.
 *   ac_lm_embed            out [B][P + T][dim]: P prompt rows (projected by prompt.weight when prompt_width == prompt_dim, copied when
 *                          it is dim) followed by the rows of toks [B][T] int64: token j reads row tok + ((curr_pos + j) % num_codebooks)
 *                          * vocab_size of the table.  Ids are clamped into the table.
 *   ac_lm_forward          appends the T rows embs [B][T][dim] at the state's position, which has to be `pos` (the host's copy), and leaves
 *                          the last row's logits pending in the state; logits_out [B][T][vocab] or NULL; the row at absolute position
 *                          p uses output head p % num_codebooks.  pos + T > capacity is AC_EINVAL and leaves the state untouched.
 *   ac_lm_step             one generated token: draws row r from the pending logits with ac_sample_tokens' top-p rule (top_p 0: argmax)
 *                          at element offset + step * B + r of the stream `key`; hyp[:, step] = tok; alive &= tok != eos_id; lens += alive;
 *                          then runs the layers on embed(tok, curr_pos = step + 1) for the next pending logits.  logits_log
 *                          [max_steps][B][vocab] or NULL receives the logits every token was drawn from.  Everything is read from the
 *                          state: a captured step replays without new arguments.  Steps behind max_steps, or behind the step in which the
 *                          last row ended, change nothing.  A step whose position would pass the capacity writes nothing and raises the
 *                          header's flag word (word 4), which the caller polls. */
typedef struct ac_lm_config {
    int32_t struct_size;
    int32_t vocab_size;        /* ids per codebook = logits per row (1026)   */
    int32_t n_layers;          /* 12                                         */
    int32_t dim;               /* 512                                        */
    int32_t ffn_dim;           /* 2048                                       */
    int32_t n_heads;           /* 4                                          */
    int32_t n_kv_heads;        /* 1                                          */
    int32_t max_seq_len;       /* 8192: the rotary table has twice as many rows */
    int32_t prompt_dim;        /* 0: none                                    */
    int32_t num_codebooks;     /* 2                                          */
    int32_t device;
    float norm_eps;            /* 1e-6                                       */
    float rope_theta;          /* 10000 (informative: the table is loaded)   */
} ac_lm_config;
typedef struct ac_lm_layout {  /* byte offsets into a state */
    long long hdr, alive, lens, tok, logits, hyp, kv;
    long long plane_bytes;     /* layer l: K at kv + 2 l plane_bytes, V one plane behind it */
    long long total;
} ac_lm_layout;
typedef struct ac_lm_stages {  /* optional outputs of ac_lm_forward, each pointer may be NULL */
    float* q;            /* [layers][B][T][n_heads * head_dim]   rotated queries                  */
    float* attn;         /* [layers][B][T][n_heads * head_dim]   attention output (before wo)     */
    float* layer_out;    /* [layers][B][T][dim]                  the layer's output               */
    float* final_norm;   /* [B][T][dim]                          the final RMSNorm                */
} ac_lm_stages;
int ac_lm_create(const ac_lm_config* cfg, ac_handle** out);
int ac_lm_state_layout(const ac_handle* h, int B, int capacity, int max_steps, ac_lm_layout* out);
size_t ac_lm_state_bytes(const ac_handle* h, int B, int capacity, int max_steps);
int ac_lm_reset(ac_handle* h, void* state_dev, size_t state_bytes, int B, int capacity, int max_steps, long long offset, void* stream);
size_t ac_lm_workspace_bytes(const ac_handle* h, int B, int T, int capacity);
int ac_lm_embed(ac_handle* h, const int64_t* toks_dev, int B, int T, int curr_pos, const float* prompt_dev, int P, int prompt_width, float* out_dev,
                void* stream);
int ac_lm_forward(ac_handle* h, void* state_dev, size_t state_bytes, int B, int capacity, int max_steps, int pos, const float* embs_dev, int T,
                  float* logits_out, const ac_lm_stages* stages, void* ws, size_t ws_bytes, void* stream);
int ac_lm_step(ac_handle* h, void* state_dev, size_t state_bytes, int B, int capacity, int max_steps, long long eos_id, float temp, float top_p,
               uint64_t key, float* logits_log, void* ws, size_t ws_bytes, void* stream);

/* Scoring token sequences teacher-forced: one causal forward over all P + T rows of every clip on the matrix
 * pipe (split16 arithmetic, per-row scales), without a state and without the 64-row limit of one.  The [B][T][vocab] logits are never
 * written: the output head keeps a running maximum, the sum of exponentials, the target's logit and the arg-max per row.
 *   ac_lm_prepare_score          once per handle before the first ac_lm_score (idempotent; SYNCHRONISES the device and reallocates the
 *                                handle's weights -- not to be called while work of the handle is in flight or being captured): packs
 *                                wq | wk | wv, wo, w1 | w3 and w2 of every layer for the tap-GEMM and the output heads for the head kernel.
 *                                The fp32 matrices of ac_lm_forward / ac_lm_step stay.  AC_EINVAL unless the matrices have rows in
 *                                multiples of 64 or 96 and columns in multiples of 32, the head dim is a multiple of 16 up to 128 and
 *                                dim <= 2048.
 *   ac_lm_score_workspace_bytes  for B clips of T_total = P + T rows: the clips of one pass are capped so that it stays near 1 GiB.
 *   ac_lm_score                  embs [B][P + T][dim] (ac_lm_embed's output), targets [B][T] int64, lengths [B] int64 or NULL.  Position t
 *                                of clip b is scored against targets[b][t] from the logits of row P + t (output head t % num_codebooks;
 *                                P has to be a multiple of num_codebooks) when the target lies in [0, vocab_size) and t < lengths[b]
 *                                (clamped into 0..T).  logp [B][T] = log_softmax(logits)[target], 0 where unscored; pred [B][T] int64 the
 *                                arg-max of every position, the lowest index on a tie; sum_logp [B] fp64 the scored log-probs summed in
 *                                a fixed order, count [B] and errors [B] int64 the scored positions and those with pred != target.  The
 *                                batch is walked in chunks of as many whole clips as `ws_bytes` holds; a clip's results do not depend on
 *                                the chunking.  Nothing is read back and nothing synchronises: the call may be captured. */
typedef struct ac_lm_score_stages {  /* optional outputs of ac_lm_score, each pointer may be NULL */
    float* q;            /* [layers][B][P + T][n_heads * head_dim]      rotated queries              */
    float* k;            /* [layers][B][P + T][n_kv_heads * head_dim]   rotated keys                 */
    float* attn;         /* [layers][B][P + T][n_heads * head_dim]      attention output (before wo) */
    float* layer_out;    /* [layers][B][P + T][dim]                     the layer's output           */
    float* final_norm;   /* [B][P + T][dim]                             the final RMSNorm            */
    float* logits;       /* [B][T][vocab]                               the logits of the token rows */
} ac_lm_score_stages;
int ac_lm_prepare_score(ac_handle* h);
size_t ac_lm_score_workspace_bytes(const ac_handle* h, int B, int T_total);
int ac_lm_score(ac_handle* h, const float* embs_dev, int B, int P, int T, const int64_t* targets_dev, const int64_t* lengths_dev, float* logp_out,
                int64_t* pred_out, double* sum_logp_out, int64_t* count_out, int64_t* errors_out, const ac_lm_score_stages* stages, void* ws,
                size_t ws_bytes, void* stream);

/* TokenProbe: the downstream recipes' probe over codec tokens -- multi-codebook embedding and pooling, a
 * bidirectional LSTM over packed sequences, and a CTC head with greedy decode or an utterance head over masked statistics pooling.
 * One more handle kind: ac_probe_create, ac_load_weights under the names below, ac_finalize, then ac_probe_forward; ac_destroy frees it.
 * AC_EINVAL from ac_probe_create unless hidden_size is a multiple of 32 up to 1024, embedding_dim (the input width) a multiple of 32,
 * num_layers in 1..8, num_codebooks in 1..32 and the enumerations are known; ac_finalize refuses exact-product arithmetic
 * (AC_PRECISION_FP32_EXACT): the input projections run as split16 row-mode GEMMs only.
 * Tensors (fp32): "embedding.weight" [K C (+ 1 with padding_idx)][E]; AC_PROBE_POOL_LINEAR: "pooling.mlp.weight" [K] (absent with K = 1);
 * AC_PROBE_POOL_ATTENTIONAL: "pooling.score" [K C + 2], the score w2 . relu(W1 e + b1) of every table row folded by the caller, entry K C
 * the padding row's and entry K C + 1 a zero row's; "encoder.rnn.{weight_ih,weight_hh,bias_ih,bias_hh}_l<n>" and "..._l<n>_reverse";
 * "head.weight" [num_classes][2H] (CTC) or [num_classes][4H] (utterance: mean columns, then std columns), "head.bias".
 *   ac_probe_workspace_bytes  for B clips of N frames: the clips of one pass are capped so that it stays near 1 GiB.
 *   ac_probe_forward          input: int64 ids [B][N][K], or fp32 features [B][N][E] with AC_PROBE_POOL_NONE.  lengths [B] int64 absolute
 *                             frame counts or NULL (all N), clamped into 0..N on the device.  An id equal to vocab_size with padding_idx
 *                             reads row K C; any other id outside [0, vocab_size) reads a zero row, indexes nothing and raises the handle's
 *                             sticky bad-token word (reported by the next entry point or ac_poll_status).  The backward direction of clip b
 *                             starts at frame lengths[b] - 1; frames beyond a length are zero in every layer output.  The batch is walked
 *                             in chunks of as many whole clips as `ws_bytes` holds; a clip's results do not depend on its batch or the
 *                             chunking.  Nothing is read back and nothing synchronises: the call may be captured. */
enum { AC_PROBE_POOL_NONE = 0, AC_PROBE_POOL_LINEAR = 1, AC_PROBE_POOL_ATTENTIONAL = 2 };
enum { AC_PROBE_HEAD_CTC = 0, AC_PROBE_HEAD_UTTERANCE = 1 };
typedef struct ac_probe_config {
    int32_t struct_size;      /* sizeof(ac_probe_config) */
    int32_t vocab_size;       /* C: ids per codebook (ignored with AC_PROBE_POOL_NONE) */
    int32_t num_codebooks;    /* K */
    int32_t embedding_dim;    /* E: the LSTM's input width */
    int32_t hidden_size;      /* H per direction */
    int32_t num_layers;
    int32_t pooling;          /* AC_PROBE_POOL_* */
    int32_t head;             /* AC_PROBE_HEAD_* */
    int32_t num_classes;
    int32_t blank_id;         /* CTC */
    int32_t padding_idx;      /* 0 / 1: the table has the extra row K C, read by the id vocab_size */
    int32_t device;
} ac_probe_config;
typedef struct ac_probe_outputs {  /* CTC: frame_pred, hyp_toks, hyp_lens required; utterance: log_probs, pred required; the rest may be NULL */
    int64_t* frame_pred;   /* CTC [B][N]: per-frame arg-max (lowest index on a tie), -1 beyond the length                    */
    int64_t* hyp_toks;     /* CTC [B][N]: repeats collapsed, blanks removed, left-packed, -1 filled                         */
    int64_t* hyp_lens;     /* CTC [B]                                                                                       */
    float* log_probs;      /* CTC [B][N][num_classes] (optional; zero beyond the length); utterance [B][num_classes]         */
    int64_t* pred;         /* utterance [B]                                                                                 */
    float* pooled;         /* stage [B][N][E]: the pooled embeddings (ignored with AC_PROBE_POOL_NONE)                      */
    float* layer_out;      /* stage [layers][B][N][2H]                                                                      */
    float* logits;         /* stage: CTC [B][N][num_classes], utterance [B][num_classes]                                    */
} ac_probe_outputs;
int ac_probe_create(const ac_probe_config* cfg, ac_handle** out);
size_t ac_probe_workspace_bytes(const ac_handle* h, int B, int N);
int ac_probe_forward(ac_handle* h, const void* input_dev, int B, int N, const int64_t* lengths_dev, const ac_probe_outputs* out, void* ws,
                     size_t ws_bytes, void* stream);

/* Optional per-kernel timing with HIP events on the caller's stream (bench.py's roofline leg).
 * ac_profile_begin arms it; every launch made by subsequent calls is bracketed by events.
 * ac_profile_end synchronises those events and writes up to `cap` records; returns the count. */
typedef struct ac_kernel_stat {
    char name[96];       /* kernel (family) name as it appears in rocprofv3 --kernel-trace; with the
                          * environment variable AC_PROF_DETAIL=1 the tap-GEMM records also carry their shape */
    int32_t launches;
    float total_ms;
    double flops;        /* algorithmic flops of those launches (2*M*N*K, ...)             */
    double bytes;        /* algorithmic HBM bytes (inputs read once + outputs written once) */
} ac_kernel_stat;
int ac_profile_begin(ac_handle* h);
int ac_profile_end(ac_handle* h, ac_kernel_stat* out, int cap);

/* Test hook: while armed (buf_dev != NULL), ac_encode/ac_encode_feats/ac_decode append every module
 * output -- in HF module order, standard channels-last [B][L][C] layout -- to buf_dev.
 * ac_debug_captured returns the floats appended so far (may exceed cap_floats: nothing is written
 * past the capacity).  Disarm with ac_debug_capture(h, NULL, 0).
 * A Mimi stream push (ac_mimi_stream_encode / _decode and their _slots forms) emits, while armed, the sub-layer outputs of its
 * transformer as dense [B][T] rows, B the rows of the native call (n of a slot push), T = F * resample_stride, A = heads * head_dim:
 *   encode:  the transformer's input [B][T][hidden];
 *   decode:  the dequantised rows [B][F][hidden], then the up-sampler's output = the transformer's input [B][T][hidden];
 *   then per layer, in order:  qkv [B][T][3A] (rotated q | rotated k | v),  att [B][T][A] (before o_proj),  the layer's output
 *   [B][T][hidden].
 * These are stream-ordered copies: the push's tokens or samples are the bits of a push without the hook. */
int ac_debug_capture(ac_handle* h, float* buf_dev, size_t cap_floats);
/* Developer / test switches of a handle: A/B paths whose results are EQUIVALENT (bit-identical or fp32-faithful; named in the
 * parity tests): "tap_epi_staged", "tap_dil", "tap_stagger", "tap_pick", "tap8", "tap8_form", "tap8_spread", "rb_stream",
 * "rb128_stream", "rb256_fused", "chain_stream", "front_seg", "tail_seg", "front_ldspad", "lstm_fuse_in", "rvq_exact", "prof_detail", "head_seq", "attn_exact",
 * "dac_unit", "mimi_tail", "mstream_skinny" (the linear layers of an ac_mimi_stream_decode push: 0 = tap-GEMM, 1 = the weight-streaming
 * mstream_linear_kernel wherever the shape allows, -1 = by rows per launch).  Their initial values come from the environment variables of the same meaning (AC_TAP_EPI, AC_TAP_DIL,
 * ...), read ONCE, at ac_finalize; no compute entry point reads the environment.
 * "rb6_dbg" (timing modes with WRONG results) and "lstm_dbg" (fault injection, traces) exist in the DEVELOPER library only
 * (libaudiocodecs_amd_dev.so, built beside the product by csrc/build.sh with -DAC_DEVELOPER): the product library returns AC_EINVAL for
 * them, does not read AC_RB6_DBG / AC_LSTM_DBG, and its kernels ignore the words.  Not part of the product interface. */
int ac_debug_set(ac_handle* h, const char* key, int value);
size_t ac_debug_captured(const ac_handle* h);

/* Test hook: the constants of the BOUNDS that stand in for an amax where a tensor exists only inside a fused kernel
 * (csrc/enc_front.h, dec_tail.h, rb_fused6.h): a split16 scale derived from a bound 2^w too large costs w of the 16 bits of
 * range split16 keeps below a tensor's largest element (csrc/split16.h); tests/test_split16_gpu.py measures w on speech-like
 * data.  Writes 11 + 4 * AC_MAX_RATIOS floats (layout at the definition, csrc/ac_api.hip) and returns that count. */
int ac_debug_bounds(const ac_handle* h, float* out, int cap);

/* Diagnostics (SYNCHRONISES): shader clock the tap_gemm6 workgroups ran at since the last call -- every workgroup reads
 * s_memtime (shader clock) and s_memrealtime (100 MHz) at its start and end; *shader_mhz = 100 * sum / sum (0 when nothing ran).
 * enable != 0 arms the sampling for the following calls, 0 disarms it.  The matrix pipe on this chip is power-capped: the
 * clock under a GEMM is the missing half of its roofline. */
int ac_debug_clock(ac_handle* h, int enable, double* shader_mhz);
/* Developer builds only (-DT6_TRACE, tools/experiments/r3o_trace.py): copies the s_memtime stage stamps one tap_gemm6 workgroup
 * left behind the clock words (ac_debug_clock must be enabled); returns the number of 64-bit words written.  SYNCHRONISES. */
int ac_debug_trace(ac_handle* h, unsigned long long* out, int words);

/* Test hook (no GPU): the host-side packer's split of ONE weight row in split16 arithmetic (csrc/split16.h): the row's scale
 * exponent s (|w| 2^s < 2^15, chosen from the row's largest magnitude), and per element the fp16 bit patterns of
 * hi = fp16_rn(w 2^s) and lo = fp16_rn(w 2^s - hi).  Returns s.  The CPU tests compare it with numpy's float16. */
int ac_debug_split_row(const float* w, int n, uint16_t* hi, uint16_t* lo);

/* Test hook (no GPU, no handle): the kernel csrc/core.hip run_tap launches for one tap-GEMM (every conv / linear layer), from
 * the inputs its routing reads (csrc/tap_route.h route_tap).  Pointer fields take 0 = null, 1 = 16-byte aligned, 2 = set but not
 * 16-byte aligned; the switch fields start from the defaults of ac_debug_set's keys of the same names (tap_dil = 1, tap_pick = -1,
 * tap8 = -1, tap8_spread = 1, the others 0).  Writes the profile record name without the shape suffix (e.g.
 * "tap_gemm6_kernel<1, 4, 4, 1, 2>") to name[cap] and sets *flags: 1 = split16 row mode, 2 = direct epilogue, 4 = rejected
 * (more than 8 taps; name empty), 8 = tap_gemm8's requests dealt between its MFMA units (SPREAD).  Returns AC_OK, or AC_EINVAL
 * for a bad query. */
typedef struct ac_tap_seg_query {
    int32_t x;                         /* pointer: the segment's input                             */
    int32_t rel_len;                   /* pointer: per-clip relative lengths                       */
    int32_t L, cin, s, J, dil, pad, lim, kofs, elu;
    int64_t bs, ts;                    /* batch / time-step strides (floats)                      */
} ac_tap_seg_query;
typedef struct ac_tap_route_query {
    int32_t struct_size;               /* = sizeof(ac_tap_route_query)                             */
    int32_t B, M, N, Ktot, nseg;       /* nseg: 1 or 2                                             */
    ac_tap_seg_query seg[2];
    int32_t w, y, y_elu, scale, res, alpha;          /* pointers                                   */
    int32_t gelu, tanh_out, n_valid;
    int64_t y_bs, y_rs, res_rs, y_off, y_len;
    int32_t has_w6, has_winv;          /* the packer made split16 planes / per-row scales of the weights */
    int32_t want_rowmode, want_rows;   /* the caller asks for row mode / for the output's row words */
    int32_t gemm_fp32;                 /* exact-fp32 products                                      */
    int32_t tap_epi_staged, tap_dil, tap_pick, tap8, tap8_form, tap8_spread;
} ac_tap_route_query;
int ac_debug_tap_route(const ac_tap_route_query* q, char* name, int cap, int32_t* flags);

/* Which LSTM path the handle uses (SYNCHRONISES the device; tests / diagnostics): 1 = the persistent single-launch kernel
 * (D = 512, 2 layers, 256-CU device; opt out with the environment variable AC_LSTM=step), 0 = one launch per
 * time step, AC_EHIP = a persistent launch failed since the handle was created (a bounded wait expired, or the launch
 * did not get 32 workgroups on every XCD -- e.g. a shared GPU).
 *
 * Failures only the device can see are STICKY and reported by the next entry point called on the handle (no entry point
 * synchronises): the failed call's outputs were set to NaN on the device -- never left unwritten --, the next call
 * returns AC_EHIP once and the handle switches to the per-step LSTM kernels; likewise a token id outside
 * [0, codebook_size) in ac_decode / ac_dequantize sets that frame to NaN and the next call returns AC_EINVAL once
 * (torch.nn.functional.embedding raises).  A clip whose samples contain NaN/Inf does not disturb the other clips of
 * the batch: its LSTM outputs are NaN from that frame on, like the reference's. */
int ac_lstm_status(ac_handle* h);

/* Explicit poll for those sticky device-side failures (round-2 advisor finding: otherwise an unrelated, correct later call is
 * the one that raises).  SYNCHRONISES `stream`, then returns what the next entry point would have returned -- AC_EHIP (a
 * persistent LSTM launch failed; the handle has switched to the per-step kernels), AC_EINVAL (token ids out of range) or AC_OK --
 * and clears the words, so that later calls are not affected.  The Python wrappers call it after each of their own calls when
 * constructed with strict=True. */
int ac_poll_status(ac_handle* h, void* stream);

const char* ac_last_error(const ac_handle* h);
void ac_destroy(ac_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* AUDIOCODECS_AMD_H */
