"""ctypes binding of libaudiocodecs_amd.so (include/audiocodecs_amd.h).

The shared library is the product; there is NO fallback: if it is missing, or no gfx950 device is
visible, every compute entry point raises.  `import torch` must precede the load so that the HIP
runtime torch already mapped (libamdhip64.so.7) is the one the library binds to.
"""

from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (loads libamdhip64 first)

__all__ = ["lib", "lib_path", "AcConfig", "AcMimiConfig", "AcDacConfig", "AcWavtokConfig", "AcVocosConfig", "AcSpkConfig", "AcSpkStages", "AcLmConfig", "AcLmLayout", "AcLmStages", "AcLmScoreStages", "AcProbeConfig", "AcProbeOutputs", "AcKernelStat", "NativeError", "check", "EXPORTS", "track", "set_precision", "check_precision", "PRECISIONS",
           "Handle", "HandleOwner"]

AC_MAX_RATIOS = 8
# AUDIOCODECS_AMD_LIB: developer override (timing variants built by hand); the product is the in-tree library
lib_path = os.environ.get("AUDIOCODECS_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libaudiocodecs_amd.so")


class NativeError(RuntimeError):
    pass


class AcConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("sampling_rate", C.c_int32),
        ("num_filters", C.c_int32),
        ("hidden_size", C.c_int32),
        ("num_ratios", C.c_int32),
        ("upsampling_ratios", C.c_int32 * AC_MAX_RATIOS),
        ("kernel_size", C.c_int32),
        ("last_kernel_size", C.c_int32),
        ("residual_kernel_size", C.c_int32),
        ("compress", C.c_int32),
        ("num_lstm_layers", C.c_int32),
        ("codebook_size", C.c_int32),
        ("num_quantizers", C.c_int32),
        ("device", C.c_int32),
    ]


class AcMimiConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("sampling_rate", C.c_int32),
        ("num_filters", C.c_int32),
        ("hidden_size", C.c_int32),
        ("num_ratios", C.c_int32),
        ("upsampling_ratios", C.c_int32 * AC_MAX_RATIOS),
        ("kernel_size", C.c_int32),
        ("last_kernel_size", C.c_int32),
        ("residual_kernel_size", C.c_int32),
        ("compress", C.c_int32),
        ("codebook_size", C.c_int32),
        ("codebook_dim", C.c_int32),
        ("num_quantizers", C.c_int32),
        ("num_semantic_quantizers", C.c_int32),
        ("num_hidden_layers", C.c_int32),
        ("num_attention_heads", C.c_int32),
        ("head_dim", C.c_int32),
        ("intermediate_size", C.c_int32),
        ("sliding_window", C.c_int32),
        ("resample_stride", C.c_int32),
        ("device", C.c_int32),
        ("rope_theta", C.c_float),
        ("norm_eps", C.c_float),
    ]


AC_MAX_DILATIONS = 4


class AcDacConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("sampling_rate", C.c_int32),
        ("encoder_hidden_size", C.c_int32),
        ("decoder_hidden_size", C.c_int32),
        ("num_ratios", C.c_int32),
        ("downsampling_ratios", C.c_int32 * AC_MAX_RATIOS),
        ("upsampling_ratios", C.c_int32 * AC_MAX_RATIOS),
        ("n_codebooks", C.c_int32),
        ("codebook_size", C.c_int32),
        ("codebook_dim", C.c_int32),
        ("num_dilations", C.c_int32),
        ("dilations", C.c_int32 * AC_MAX_DILATIONS),
        ("device", C.c_int32),
    ]


class AcWavtokConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("sampling_rate", C.c_int32),
        ("num_filters", C.c_int32),
        ("dimension", C.c_int32),
        ("num_ratios", C.c_int32),
        ("ratios", C.c_int32 * AC_MAX_RATIOS),
        ("kernel_size", C.c_int32),
        ("last_kernel_size", C.c_int32),
        ("residual_kernel_size", C.c_int32),
        ("compress", C.c_int32),
        ("num_lstm_layers", C.c_int32),
        ("codebook_size", C.c_int32),
        ("backbone_dim", C.c_int32),
        ("intermediate_dim", C.c_int32),
        ("num_layers", C.c_int32),
        ("adanorm_num_embeddings", C.c_int32),
        ("num_groups", C.c_int32),
        ("n_fft", C.c_int32),
        ("bandwidth_id", C.c_int32),
        ("device", C.c_int32),
    ]


class AcVocosConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("input_channels", C.c_int32),
        ("codebook_size", C.c_int32),
        ("max_codebooks", C.c_int32),
        ("backbone_dim", C.c_int32),
        ("intermediate_dim", C.c_int32),
        ("num_layers", C.c_int32),
        ("adanorm_num_embeddings", C.c_int32),
        ("n_fft", C.c_int32),
        ("hop_length", C.c_int32),
        ("bandwidth_id", C.c_int32),
        ("device", C.c_int32),
    ]


class AcSpkConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("conv_dim", C.c_int32),
        ("num_conv_layers", C.c_int32),
        ("conv_kernel", C.c_int32 * AC_MAX_RATIOS),
        ("conv_stride", C.c_int32 * AC_MAX_RATIOS),
        ("hidden_size", C.c_int32),
        ("num_hidden_layers", C.c_int32),
        ("num_attention_heads", C.c_int32),
        ("intermediate_size", C.c_int32),
        ("num_conv_pos_embeddings", C.c_int32),
        ("num_conv_pos_embedding_groups", C.c_int32),
        ("num_buckets", C.c_int32),
        ("max_bucket_distance", C.c_int32),
        ("num_tdnn_layers", C.c_int32),
        ("tdnn_dim", C.c_int32 * AC_MAX_RATIOS),
        ("tdnn_kernel", C.c_int32 * AC_MAX_RATIOS),
        ("tdnn_dilation", C.c_int32 * AC_MAX_RATIOS),
        ("xvector_output_dim", C.c_int32),
        ("feat_extract_norm_group", C.c_int32),
        ("conv_bias", C.c_int32),
        ("do_stable_layer_norm", C.c_int32),
        ("use_weighted_layer_sum", C.c_int32),
        ("add_adapter", C.c_int32),
        ("max_chunk_clips", C.c_int32),
        ("device", C.c_int32),
        ("layer_norm_eps", C.c_float),
    ]


class AcSpkStages(C.Structure):
    _fields_ = [("feat", C.c_void_p), ("hidden", C.c_void_p), ("tdnn", C.c_void_p), ("pooled", C.c_void_p)]


class AcLmConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32),
        ("vocab_size", C.c_int32),
        ("n_layers", C.c_int32),
        ("dim", C.c_int32),
        ("ffn_dim", C.c_int32),
        ("n_heads", C.c_int32),
        ("n_kv_heads", C.c_int32),
        ("max_seq_len", C.c_int32),
        ("prompt_dim", C.c_int32),
        ("num_codebooks", C.c_int32),
        ("device", C.c_int32),
        ("norm_eps", C.c_float),
        ("rope_theta", C.c_float),
    ]


class AcLmLayout(C.Structure):
    _fields_ = [(k, C.c_longlong) for k in ("hdr", "alive", "lens", "tok", "logits", "hyp", "kv", "plane_bytes", "total")]


class AcLmStages(C.Structure):
    _fields_ = [("q", C.c_void_p), ("attn", C.c_void_p), ("layer_out", C.c_void_p), ("final_norm", C.c_void_p)]


class AcLmScoreStages(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("q", "k", "attn", "layer_out", "final_norm", "logits")]


class AcProbeConfig(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("struct_size", "vocab_size", "num_codebooks", "embedding_dim", "hidden_size", "num_layers", "pooling", "head", "num_classes",
                                         "blank_id", "padding_idx", "device")]


class AcProbeOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("frame_pred", "hyp_toks", "hyp_lens", "log_probs", "pred", "pooled", "layer_out", "logits")]


class AcKernelStat(C.Structure):
    _fields_ = [
        ("name", C.c_char * 96),
        ("launches", C.c_int32),
        ("total_ms", C.c_float),
        ("flops", C.c_double),
        ("bytes", C.c_double),
    ]


_vp, _i, _sz, _ll = C.c_void_p, C.c_int, C.c_size_t, C.c_longlong
# name -> (restype, argtypes): every symbol include/audiocodecs_amd.h declares
EXPORTS = {
    "ac_version": (_i, []),
    "ac_create": (_i, [C.POINTER(AcConfig), C.POINTER(_vp)]),
    "ac_mimi_create": (_i, [C.POINTER(AcMimiConfig), C.POINTER(_vp)]),
    "ac_dac_create": (_i, [C.POINTER(AcDacConfig), C.POINTER(_vp)]),
    "ac_wavtok_create": (_i, [C.POINTER(AcWavtokConfig), C.POINTER(_vp)]),
    "ac_vocos_create": (_i, [C.POINTER(AcVocosConfig), C.POINTER(_vp)]),
    "ac_decode_feats": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_load_weights": (_i, [_vp, C.c_char_p, _vp, _sz]),
    "ac_set_precision": (_i, [_vp, _i]),
    "ac_finalize": (_i, [_vp]),
    "ac_num_frames": (_i, [_vp, _i]),
    "ac_num_samples": (C.c_longlong, [_vp, _i]),
    "ac_hop_length": (_i, [_vp]),
    "ac_hidden_size": (_i, [_vp]),
    "ac_codebook_dim": (_i, [_vp]),
    "ac_encode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_decode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_encode": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_encode_feats": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_decode": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_quantize": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "ac_dequantize": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "ac_encode_quantized": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "ac_encode_feats_latent": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_quantizer_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_quantize_ws": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_dequantize_ws": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_mimi_stream_state_bytes": (_sz, [_vp, _i]),
    "ac_mimi_stream_reset": (_i, [_vp, _vp, _sz, _i, _vp, _vp]),
    "ac_mimi_stream_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_mimi_stream_encode": (_i, [_vp, _vp, _sz, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_mimi_stream_decode_state_bytes": (_sz, [_vp, _i]),
    "ac_mimi_stream_decode_reset": (_i, [_vp, _vp, _sz, _i, _vp, _vp]),
    "ac_mimi_stream_decode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_mimi_stream_decode": (_i, [_vp, _vp, _sz, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_mimi_stream_encode_slots": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_mimi_stream_decode_slots": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_encodec_stream_state_bytes": (_sz, [_vp, _i]),
    "ac_encodec_stream_reset": (_i, [_vp, _vp, _sz, _i, _vp, _vp]),
    "ac_encodec_stream_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_encodec_stream_encode": (_i, [_vp, _vp, _sz, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_encodec_stream_decode_state_bytes": (_sz, [_vp, _i]),
    "ac_encodec_stream_decode_reset": (_i, [_vp, _vp, _sz, _i, _vp, _vp]),
    "ac_encodec_stream_decode_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_encodec_stream_decode": (_i, [_vp, _vp, _sz, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_encodec_stream_reset_slots": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _i, _vp]),
    "ac_encodec_stream_decode_reset_slots": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _i, _vp]),
    "ac_encodec_stream_encode_slots": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_encodec_stream_decode_slots": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_embs": (_i, [_vp, _i, _vp, _vp]),
    "ac_embs_projected": (_i, [_vp, _i, _vp, _vp]),
    "ac_resample": (_i, [_vp, _i, _i, _vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "ac_resample_stream_out_len": (_ll, [_ll, _i, _i, _i, _i, _i]),
    "ac_resample_stream_state_bytes": (_sz, [_i, _i]),
    "ac_resample_stream_reset": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "ac_resample_stream_push": (_i, [_vp, _sz, _vp, _ll, _i, _i, _ll, _vp, _i, _i, _i, _i, _vp, _ll, _ll, _i, _vp]),
    "ac_resample_stream_reset_slots": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "ac_resample_stream_push_slots": (_i, [_vp, _sz, _i, _vp, _vp, _vp, _vp, _i, _vp, _ll, _i, _vp, _i, _i, _i, _i, _vp, _ll, _ll, _i, _vp]),
    "ac_knn_packed_bytes": (_sz, [_ll, _i]),
    "ac_knn_pack": (_i, [_vp, _ll, _i, _vp, _sz, _vp]),
    "ac_knn_num_splits": (_i, [_ll, _ll, _i, _i]),
    "ac_knn_workspace_bytes": (_sz, [_ll, _ll, _i, _i, _i]),
    "ac_knn_match": (_i, [_vp, _ll, _vp, _vp, _ll, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ac_specdist_source_count": (_sz, []),
    "ac_specdist_source": (_i, [_vp, _sz]),
    "ac_specdist_tables_bytes": (_sz, []),
    "ac_specdist_tables": (_i, [_vp, _vp, _sz, _vp]),
    "ac_specdist_num_frames": (_ll, [_ll]),
    "ac_specdist_workspace_bytes": (_sz, [_i, _ll, _ll]),
    "ac_specdist": (_i, [_vp, _vp, _i, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ac_stoi_source_count": (_sz, []),
    "ac_stoi_source": (_i, [_vp, _sz]),
    "ac_stoi_tables_bytes": (_sz, []),
    "ac_stoi_tables": (_i, [_vp, _vp, _sz, _vp]),
    "ac_stoi_num_frames": (_ll, [_ll]),
    "ac_stoi_workspace_bytes": (_sz, [_i, _ll, _ll]),
    "ac_stoi": (_i, [_vp, _vp, _i, _ll, _ll, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ac_dnsmos_source_count": (_sz, []),
    "ac_dnsmos_source": (_i, [_vp, _sz]),
    "ac_dnsmos_tables_bytes": (_sz, []),
    "ac_dnsmos_tables": (_i, [_vp, _vp, _sz, _vp]),
    "ac_dnsmos_weights_count": (_sz, []),
    "ac_dnsmos_packed_bytes": (_sz, []),
    "ac_dnsmos_pack": (_i, [_vp, _sz, _vp, _sz, _vp]),
    "ac_dnsmos_workspace_bytes": (_sz, [_ll, _i, _i]),
    "ac_dnsmos_net": (_i, [_vp, _ll, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ac_dnsmos": (_i, [_vp, _ll, _ll, _vp, _ll, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "ac_tokstats_state_bytes": (_sz, [_i, _i]),
    "ac_tokstats_form": (_i, [_i, _i]),
    "ac_tokstats_accumulate": (_i, [_vp, _ll, _ll, _i, _i, _vp, _vp, _sz, _vp]),
    "ac_tokstats_summary": (_i, [_vp, _i, _i, _vp, _vp]),
    "ac_sample_form": (_i, [_i]),
    "ac_sample_tokens": (_i, [_vp, _ll, _vp, _ll, _i, C.c_float, _i, C.c_float, C.c_uint64, C.c_uint64, _vp, C.c_float, _vp, _vp, _vp]),
    "ac_spk_create": (_i, [C.POINTER(AcSpkConfig), C.POINTER(_vp)]),
    "ac_spk_num_frames": (_i, [_ll]),
    "ac_spk_workspace_bytes": (_sz, [_vp, _i, _ll]),
    "ac_spk_embed": (_i, [_vp, _vp, _vp, _i, _ll, _vp, C.POINTER(AcSpkStages), _vp, _sz, _vp]),
    "ac_spk_cosine": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ac_lm_create": (_i, [C.POINTER(AcLmConfig), C.POINTER(_vp)]),
    "ac_lm_state_layout": (_i, [_vp, _i, _i, _i, C.POINTER(AcLmLayout)]),
    "ac_lm_state_bytes": (_sz, [_vp, _i, _i, _i]),
    "ac_lm_reset": (_i, [_vp, _vp, _sz, _i, _i, _i, _ll, _vp]),
    "ac_lm_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "ac_lm_embed": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _i, _vp, _vp]),
    "ac_lm_forward": (_i, [_vp, _vp, _sz, _i, _i, _i, _i, _vp, _i, _vp, C.POINTER(AcLmStages), _vp, _sz, _vp]),
    "ac_lm_step": (_i, [_vp, _vp, _sz, _i, _i, _i, _ll, C.c_float, C.c_float, C.c_uint64, _vp, _vp, _sz, _vp]),
    "ac_lm_prepare_score": (_i, [_vp]),
    "ac_lm_score_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_lm_score": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(AcLmScoreStages), _vp, _sz, _vp]),
    "ac_probe_create": (_i, [C.POINTER(AcProbeConfig), C.POINTER(_vp)]),
    "ac_probe_workspace_bytes": (_sz, [_vp, _i, _i]),
    "ac_probe_forward": (_i, [_vp, _vp, _i, _i, _vp, C.POINTER(AcProbeOutputs), _vp, _sz, _vp]),
    "ac_profile_begin": (_i, [_vp]),
    "ac_profile_end": (_i, [_vp, C.POINTER(AcKernelStat), _i]),
    "ac_debug_clock": (_i, [_vp, _i, C.POINTER(C.c_double)]),
    "ac_debug_bounds": (_i, [_vp, C.POINTER(C.c_float), _i]),
    "ac_debug_trace": (_i, [_vp, C.POINTER(C.c_ulonglong), _i]),
    "ac_debug_split_row": (_i, [_vp, _i, _vp, _vp]),
    "ac_debug_tap_route": (_i, [_vp, C.c_char_p, _i, C.POINTER(C.c_int32)]),
    "ac_debug_capture": (_i, [_vp, _vp, _sz]),
    "ac_debug_set": (_i, [_vp, C.c_char_p, _i]),
    "ac_debug_captured": (_sz, [_vp]),
    "ac_lstm_status": (_i, [_vp]),
    "ac_poll_status": (_i, [_vp, _vp]),
    "ac_last_error": (C.c_char_p, [_vp]),
    "ac_destroy": (None, [_vp]),
}

PRECISIONS = {"fp32": 0, "fp32_exact": 1}   # AC_PRECISION_*


def check_precision(precision):
    if precision is not None and precision not in PRECISIONS:
        raise ValueError(f"`precision` ({precision}) must be one of {list(PRECISIONS)}")
    return precision


def set_precision(L, h, precision) -> None:
    """precision: None (library default / AC_GEMM), "fp32" (split16: fp32 fidelity on the fp16 matrix pipe), "fp32_exact" (IEEE fp32 products)."""
    if precision is None:
        return
    if precision not in PRECISIONS:
        raise ValueError(f"`precision` ({precision}) must be one of {list(PRECISIONS)}")
    check(L.ac_set_precision(h, PRECISIONS[precision]), h, "ac_set_precision")


def debug_set(codec, key: str, value: int) -> None:
    """Developer / test switch on every live handle of a wrapper (include/audiocodecs_amd.h ac_debug_set).  Handles are created
    lazily per device: call the wrapper (or `codec._native_for(tensor)`) first.  Switches start from the environment variables of
    the same meaning, which the library reads once per handle at ac_finalize."""
    if not codec._natives:
        raise NativeError("debug_set: the wrapper has no handle yet (call it, or _native_for(tensor), first)")
    for nat in codec._natives.values():
        check(nat.lib.ac_debug_set(nat.h, key.encode(), int(value)), nat.h, "ac_debug_set")


_lib = None
_live = None   # weak set of objects holding an ac_handle (attribute `h`): destroyed at interpreter exit, while the HIP
               # runtime is still up (a handle owns device memory, pinned host memory and events)


def track(obj) -> None:
    """Register an object with attributes `lib` and `h` (an ac_handle) for destruction at exit."""
    global _live
    if _live is None:
        import atexit
        import weakref

        _live = weakref.WeakSet()

        def _destroy_all():
            for o in list(_live):
                try:
                    if getattr(o, "h", None):
                        o.lib.ac_destroy(o.h)
                        o.h = None
                except Exception:
                    pass

        atexit.register(_destroy_all)
    _live.add(obj)


def lib():
    """Load (once) and return the library; raises NativeError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(lib_path):
            raise NativeError(
                f"{lib_path} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()' or audiocodecs_amd/csrc/build.sh)"
            )
        L = C.CDLL(lib_path)
        for name, (res, args) in EXPORTS.items():
            fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, handle=None, what: str = "") -> None:
    if rc < 0:
        msg = lib().ac_last_error(handle).decode() if handle else ""
        raise NativeError(f"{what} failed with code {rc}: {msg}")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Handle:
    """One ac_handle: weights on one GPU + a grow-only workspace tensor.  `create` names the codec's `ac_*create`, `cfg` is its config
    struct with the architecture filled in (struct_size and device are set here), `hint` what a refusal most likely means; every
    floating-point tensor of `weights` is loaded under its name."""

    def __init__(self, create: str, cfg, hint: str, weights, device: torch.device, precision=None):
        self.lib = lib()
        cfg.struct_size = C.sizeof(cfg)
        cfg.device = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", cfg.device)
        self.h = C.c_void_p()
        rc = getattr(self.lib, create)(C.byref(cfg), C.byref(self.h))
        if rc < 0:
            raise NativeError(f"{create} failed with code {rc} ({hint})")
        set_precision(self.lib, self.h, precision)
        for name, t in weights.items():
            if not torch.is_tensor(t) or not t.is_floating_point():
                continue
            t = t.detach().to(torch.float32).cpu().contiguous()
            check(self.lib.ac_load_weights(self.h, name.encode(), C.c_void_p(t.data_ptr()), t.numel() * 4), self.h, f"ac_load_weights({name})")
        with torch.cuda.device(self.device):
            check(self.lib.ac_finalize(self.h), self.h, "ac_finalize")
        self.ws = None
        track(self)

    def workspace(self, nbytes: int) -> torch.Tensor:
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        return self.ws

    def __del__(self):
        try:
            import sys

            if sys.is_finalizing():   # interpreter shutdown: the HIP runtime may already be gone, the OS reclaims the rest
                return
            if getattr(self, "h", None):
                self.lib.ac_destroy(self.h)
                self.h = None
        except Exception:
            pass


class HandleOwner:
    """What the four wrappers share: one lazily created `Handle` per device in `self._natives` (device index -> handle).  A wrapper
    states only how its handle is built (`_new_handle`)."""

    def _new_handle(self, device: torch.device) -> Handle:
        raise NotImplementedError

    def _native_for(self, t: torch.Tensor) -> Handle:
        if not t.is_cuda:
            raise NativeError(
                "audiocodecs_amd runs on MI355X only: move the input to a cuda device "
                "(there is deliberately no CPU fallback)"
            )
        idx = t.device.index
        if idx not in self._natives:
            self._natives[idx] = self._new_handle(t.device)
        return self._natives[idx]

    def _any_native(self) -> Handle:
        """A handle that exists, or one on the current device."""
        dev = next(iter(self._natives.values())).device if self._natives else torch.device("cuda", torch.cuda.current_device())
        return self._native_for(torch.empty(0, device=dev))

    # ---- measurement hook used by bench.py ------------------------------------------------------
    def profile_kernels(self, fn):
        """Run fn() with per-kernel HIP-event timing armed; returns [(name, launches, ms, flops, bytes)]."""
        nats = self._profiled_handles()
        for nat in nats:
            check(nat.lib.ac_profile_begin(nat.h), nat.h, "ac_profile_begin")
        try:
            fn()
        finally:
            ends = []
            for nat in nats:
                buf = (AcKernelStat * 256)()
                ends.append((nat, buf, nat.lib.ac_profile_end(nat.h, buf, 256)))
        out = []
        for nat, buf, n in ends:
            check(n, nat.h, "ac_profile_end")
            out += [(buf[i].name.decode(), buf[i].launches, buf[i].total_ms, buf[i].flops, buf[i].bytes) for i in range(n)]
        return out

    def _profiled_handles(self):
        """The handles `profile_kernels` arms: the wrapper's handle (a wrapper with a second handle map adds what exists of it)."""
        return [self._any_native()]
