"""WavLM x-vector speaker embeddings and speaker similarity: the reference's ``SpkSimWavLM`` metric
(downstream/metrics/speaker_similarity.py:72-123) and its TTS speaker encoder (downstream/models/speaker_encoder.py), both of which run
transformers' ``WavLMForXVector`` of the ``microsoft/wavlm-base-sv`` family in eager torch, as one handle kind of the HIP library
(``ac_spk_create`` / ``ac_spk_embed``): the conv front end, the transformer with WavLM's gated relative-position attention, the weighted
layer sum, the TDNN head and the statistic pooling.  There is no CPU fallback.

Only the architecture of that family is compiled: ``feat_extract_norm="group"``, no conv bias, post-LN layers, the weighted layer sum,
no adapter, head dim 64, the conv kernels (10,3,3,3,3,2,2) with strides (5,2,2,2,2,2,2).  ``WAVLM_BASE_SV`` is the real shape,
``WAVLM_SV_TINY`` a narrow model of the same topology for tests.

``SpeakerEncoder.forward(sig, sample_rate, lens)`` resamples to 16 kHz with the library's resampler, replicate-pads to 4880 samples
(the reference's rule) and returns the x-vector ``embeddings`` [B, D] (not the classifier's logits).  ``lens`` are relative lengths:
``valid = int(lens * L16)`` samples of a clip are speech; frames beyond them are zeroed behind the feature projection, masked as
attention keys and left out of the pooling, exactly as the backend does -- including that query rows beyond a clip's length still reach
the pooled rows through the TDNN's receptive field, and that a clip with one pooled row has a NaN embedding.
"""

from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Tuple

import torch

from . import _metric_host as _host
from . import _native
from ._metric_host import SAMPLE_RATE
from .metrics import _DistanceStats

__all__ = ["WavLMSVConfig", "WAVLM_BASE_SV", "WAVLM_SV_TINY", "SpeakerEncoder", "speaker_similarity", "SpkSimWavLM", "bucket_table",
           "fold_pos_conv_weight_norm", "num_frames", "num_pooled_rows", "MIN_LEN", "SAMPLE_RATE"]

MIN_LEN = 4880          # samples at 16 kHz the signal is replicate-padded to (speaker_similarity.py:96-99): 15 frames, one pooled row
TDNN_SHRINK = 14        # rows the TDNN stack drops: (5-1)*1 + (3-1)*2 + (3-1)*3


@dataclass(frozen=True)
class WavLMSVConfig:
    """Fields of the third-party ``transformers.WavLMConfig`` the speaker encoder depends on (defaults = ``microsoft/wavlm-base-sv``)."""

    conv_dim: int = 512
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    num_buckets: int = 320
    max_bucket_distance: int = 800
    tdnn_dim: Tuple[int, ...] = (512, 512, 512, 512, 1500)
    tdnn_kernel: Tuple[int, ...] = (5, 3, 3, 1, 1)
    tdnn_dilation: Tuple[int, ...] = (1, 2, 3, 1, 1)
    xvector_output_dim: int = 512
    layer_norm_eps: float = 1e-5
    feat_extract_norm: str = "group"
    conv_bias: bool = False
    do_stable_layer_norm: bool = False
    use_weighted_layer_sum: bool = True
    add_adapter: bool = False
    max_chunk_clips: int = 0      # clips per pass over the stack; 0: as many as keep the workspace under the library's cap

    def hf_kwargs(self) -> dict:
        """The keyword arguments of ``transformers.WavLMConfig`` that state this architecture."""
        return dict(conv_dim=[self.conv_dim] * len(self.conv_kernel), conv_kernel=list(self.conv_kernel), conv_stride=list(self.conv_stride),
                    hidden_size=self.hidden_size, num_hidden_layers=self.num_hidden_layers, num_attention_heads=self.num_attention_heads,
                    intermediate_size=self.intermediate_size, num_conv_pos_embeddings=self.num_conv_pos_embeddings,
                    num_conv_pos_embedding_groups=self.num_conv_pos_embedding_groups, num_buckets=self.num_buckets,
                    max_bucket_distance=self.max_bucket_distance, tdnn_dim=list(self.tdnn_dim), tdnn_kernel=list(self.tdnn_kernel),
                    tdnn_dilation=list(self.tdnn_dilation), xvector_output_dim=self.xvector_output_dim, layer_norm_eps=self.layer_norm_eps,
                    feat_extract_norm=self.feat_extract_norm, conv_bias=self.conv_bias, do_stable_layer_norm=self.do_stable_layer_norm,
                    use_weighted_layer_sum=self.use_weighted_layer_sum, add_adapter=self.add_adapter, hidden_act="gelu",
                    feat_extract_activation="gelu", mask_time_prob=0.05)

    @classmethod
    def from_hf(cls, config) -> "WavLMSVConfig":
        """From a ``transformers.WavLMConfig``; what the library cannot run is refused by ``ac_spk_create``."""
        dims = set(config.conv_dim)
        if len(dims) != 1 or config.hidden_act != "gelu" or config.feat_extract_activation != "gelu":
            raise ValueError("only conv layers of one width and GELU activations are compiled")
        return cls(conv_dim=int(config.conv_dim[0]), conv_kernel=tuple(config.conv_kernel), conv_stride=tuple(config.conv_stride),
                   hidden_size=config.hidden_size, num_hidden_layers=config.num_hidden_layers, num_attention_heads=config.num_attention_heads,
                   intermediate_size=config.intermediate_size, num_conv_pos_embeddings=config.num_conv_pos_embeddings,
                   num_conv_pos_embedding_groups=config.num_conv_pos_embedding_groups, num_buckets=config.num_buckets,
                   max_bucket_distance=config.max_bucket_distance, tdnn_dim=tuple(config.tdnn_dim), tdnn_kernel=tuple(config.tdnn_kernel),
                   tdnn_dilation=tuple(config.tdnn_dilation), xvector_output_dim=config.xvector_output_dim, layer_norm_eps=config.layer_norm_eps,
                   feat_extract_norm=config.feat_extract_norm, conv_bias=bool(config.conv_bias), do_stable_layer_norm=bool(config.do_stable_layer_norm),
                   use_weighted_layer_sum=bool(config.use_weighted_layer_sum), add_adapter=bool(config.add_adapter))


WAVLM_BASE_SV = WavLMSVConfig()
# Same kernels, strides, TDNN kernels and dilations; 2 heads of 64, 2 layers, a positional conv of 16 taps in 4 groups, buckets that clamp
# at 80 frames: every code path of the real shape at widths a test runs in a second.
WAVLM_SV_TINY = WavLMSVConfig(conv_dim=32, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                              num_conv_pos_embeddings=16, num_conv_pos_embedding_groups=4, num_buckets=32, max_bucket_distance=80,
                              tdnn_dim=(64, 64, 64, 64, 96), xvector_output_dim=48)


def num_frames(length_16k: int) -> int:
    """Frames of a clip of `length_16k` samples at 16 kHz: (L - 400) // 320 + 1 (no GPU)."""
    return int(_native.lib().ac_spk_num_frames(int(length_16k)))


def num_pooled_rows(length_16k: int, valid=None) -> int:
    """Rows of the last TDNN layer that the statistic pooling takes for a clip of `length_16k` samples of which `valid` are speech
    (None: no mask): T - 14 without a mask, min(Lf - 8, T - 14) with one, Lf = (valid - 400) // 320 + 1 -- the backend's length formula,
    which ignores the dilations.  May be zero or negative: such a clip has no embedding."""
    T = num_frames(length_16k)
    if valid is None:
        return T - TDNN_SHRINK
    Lf = min((int(valid) - 400) // 320 + 1, T) if valid >= 400 else 0
    return min(Lf - 8, T - TDNN_SHRINK)


def bucket_table(cfg: WavLMSVConfig) -> torch.Tensor:
    """The relative-position bucket of every offset delta = key - query in [-2 max_distance, 2 max_distance] (int64), with the backend's
    own fp32 operations (``WavLMAttention._relative_positions_bucket``) so that every bucket boundary agrees exactly; beyond the range
    the buckets are constant (they clamp at max_distance).  The library takes it as data (``spk.bucket_table``)."""
    import math

    R = 2 * cfg.max_bucket_distance
    rel = torch.arange(-R, R + 1, dtype=torch.long)
    nb = cfg.num_buckets // 2
    buckets = (rel > 0).to(torch.long) * nb
    rel = torch.abs(rel)
    max_exact = nb // 2
    is_small = rel < max_exact
    large = torch.log(rel.float() / max_exact)
    large = large / math.log(cfg.max_bucket_distance / max_exact)
    large = large * (nb - max_exact)
    large = (max_exact + large).to(torch.long)
    large = torch.min(large, torch.full_like(large, nb - 1))
    return buckets + torch.where(is_small, rel, large)


def fold_pos_conv_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """The positional conv's weight from its weight-norm parametrisation with ``dim=2``: `g` = original0 [1, 1, k], `v` = original1
    [H, H / groups, k] -> v * g / ||v|| with one norm per tap (over dims 0 and 1)."""
    return v * (g / torch.linalg.vector_norm(v, dim=(0, 1), keepdim=True))


def _struct(cfg: WavLMSVConfig) -> _native.AcSpkConfig:
    c = _native.AcSpkConfig()
    n, t = len(cfg.conv_kernel), len(cfg.tdnn_dim)
    if len(cfg.conv_stride) != n or not 1 <= n <= _native.AC_MAX_RATIOS or len(cfg.tdnn_kernel) != t or len(cfg.tdnn_dilation) != t or not 1 <= t <= _native.AC_MAX_RATIOS:
        raise ValueError("conv_kernel / conv_stride and tdnn_dim / tdnn_kernel / tdnn_dilation must be tuples of one length each (at most 8)")
    c.conv_dim, c.num_conv_layers = cfg.conv_dim, n
    for i in range(n):
        c.conv_kernel[i], c.conv_stride[i] = cfg.conv_kernel[i], cfg.conv_stride[i]
    c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.intermediate_size
    c.num_conv_pos_embeddings, c.num_conv_pos_embedding_groups = cfg.num_conv_pos_embeddings, cfg.num_conv_pos_embedding_groups
    c.num_buckets, c.max_bucket_distance, c.num_tdnn_layers = cfg.num_buckets, cfg.max_bucket_distance, t
    for i in range(t):
        c.tdnn_dim[i], c.tdnn_kernel[i], c.tdnn_dilation[i] = cfg.tdnn_dim[i], cfg.tdnn_kernel[i], cfg.tdnn_dilation[i]
    c.xvector_output_dim = cfg.xvector_output_dim
    c.feat_extract_norm_group = 1 if cfg.feat_extract_norm == "group" else 0
    c.conv_bias, c.do_stable_layer_norm = int(bool(cfg.conv_bias)), int(bool(cfg.do_stable_layer_norm))
    c.use_weighted_layer_sum, c.add_adapter = int(bool(cfg.use_weighted_layer_sum)), int(bool(cfg.add_adapter))
    c.max_chunk_clips = int(cfg.max_chunk_clips)
    c.layer_norm_eps = float(cfg.layer_norm_eps)
    return c


class SpeakerEncoder(_native.HandleOwner):
    """``WavLMForXVector`` on the HIP library.  With a `state_dict` (the model's own key layout) and its `arch`, nothing is fetched;
    without one the checkpoint `model_hub` is loaded through transformers, as the reference does.  `pool=False` returns the last hidden
    state [B, T, H] instead of the x-vector (downstream/models/speaker_encoder.py:65-68)."""

    def __init__(self, model_hub: str = "microsoft/wavlm-base-sv", *, state_dict=None, arch: WavLMSVConfig = None, pool: bool = True):
        if state_dict is None:
            from transformers import AutoModelForAudioXVector

            model = AutoModelForAudioXVector.from_pretrained(model_hub)
            state_dict = model.state_dict()
            arch = WavLMSVConfig.from_hf(model.config) if arch is None else arch
        self.arch = WAVLM_BASE_SV if arch is None else arch
        if not isinstance(self.arch, WavLMSVConfig):
            raise ValueError("`arch` must be a WavLMSVConfig")
        _struct(self.arch)       # (its refusals, before any work)
        self.pool = bool(pool)
        self._weights = {k: v for k, v in state_dict.items() if not k.startswith(("classifier.", "objective."))}
        self._weights["spk.bucket_table"] = bucket_table(self.arch).to(torch.float32)
        self._natives = {}

    def _new_handle(self, device: torch.device) -> _native.Handle:
        return _native.Handle("ac_spk_create", _struct(self.arch),
                              "only the microsoft/wavlm-base-sv family is compiled: group norm, no conv bias, post-LN, weighted layer sum, no adapter, head dim 64",
                              self._weights, device)

    @torch.no_grad()
    def embed_16k(self, sig16: torch.Tensor, valid: torch.Tensor = None, return_stages: bool = False):
        """`sig16` [B, L] fp32 at 16 kHz, raw; `valid` [B] int32 on the same device or None -> embeddings [B, D] (with `return_stages`:
        (embeddings, {"feat", "hidden", "tdnn", "pooled"})).  This is ``ac_spk_embed``: no resampling, no padding."""
        if not torch.is_tensor(sig16) or sig16.dim() != 2 or sig16.dtype != torch.float32:
            raise ValueError("`sig16` must be a [B, L] fp32 tensor")
        B, L = (int(n) for n in sig16.shape)
        if valid is not None and (not torch.is_tensor(valid) or valid.dtype != torch.int32 or tuple(valid.shape) != (B,)):
            raise ValueError(f"`valid` must be an int32 tensor of shape [{B}]")
        if L < MIN_LEN:
            raise ValueError(f"clips of {L} samples at {SAMPLE_RATE} Hz give no row to pool: at least {MIN_LEN} (pad, as `forward` does)")
        _host.need_cuda(sig16.is_cuda and (valid is None or valid.is_cuda), "spksim", "signal and the lengths")
        nat = self._native_for(sig16)
        a, dev = self.arch, sig16.device
        T, D, H, last = num_frames(L), a.xvector_output_dim, a.hidden_size, a.tdnn_dim[-1]
        emb = torch.empty(B, D, dtype=torch.float32, device=dev)
        stages, st = None, None
        if return_stages or not self.pool:
            stages = {"hidden": torch.empty(a.num_hidden_layers + 1, B, T, H, dtype=torch.float32, device=dev)}
            if return_stages:
                stages.update(feat=torch.empty(B, T, a.conv_dim, dtype=torch.float32, device=dev),
                              tdnn=torch.empty(B, T - TDNN_SHRINK, last, dtype=torch.float32, device=dev),
                              pooled=torch.empty(B, 2 * last, dtype=torch.float32, device=dev))
            st = _native.AcSpkStages(*(stages[k].data_ptr() if k in stages else None for k in ("feat", "hidden", "tdnn", "pooled")))
        if B == 0:
            return (emb, stages) if return_stages else emb
        x = sig16.contiguous()
        with torch.cuda.device(dev):
            ws = nat.workspace(int(nat.lib.ac_spk_workspace_bytes(nat.h, B, L)))
            rc = nat.lib.ac_spk_embed(nat.h, _native._ptr(x), _native._ptr(valid.contiguous() if valid is not None else None), B, L, _native._ptr(emb),
                                      C.byref(st) if st is not None else None, _native._ptr(ws), ws.numel(), _native._stream())
        _native.check(rc, nat.h, "ac_spk_embed")
        out = emb if self.pool else stages["hidden"][-1]
        return (out, stages) if return_stages else out

    @torch.no_grad()
    def forward(self, sig: torch.Tensor, sample_rate: int, lens: torch.Tensor = None, return_stages: bool = False):
        """`sig` [B, T] at `sample_rate`, `lens` [B] relative lengths in (0, 1] or None -> the x-vector embeddings [B, D] (the last hidden
        state [B, T', H] with `pool=False`); with `return_stages` also the dictionary of stage outputs."""
        _host.check_sample_rate(sample_rate)
        if not torch.is_tensor(sig) or sig.dim() != 2:
            raise ValueError("`sig` must be a [B, T] tensor")
        B = int(sig.shape[0])
        if lens is not None and (not torch.is_tensor(lens) or tuple(lens.shape) != (B,) or not lens.is_floating_point()):
            raise ValueError(f"`lens` must be a floating-point tensor of shape [{B}]: relative lengths")
        _host.resampled_len(int(sig.shape[1]), sample_rate)
        _host.need_cuda(sig.is_cuda, "spksim", "signal")
        from .resample import resample

        x = resample(sig.detach().to(torch.float32), sample_rate, SAMPLE_RATE)
        if x.shape[-1] < MIN_LEN:
            x = torch.nn.functional.pad(x, [0, MIN_LEN - x.shape[-1]], mode="replicate")
        valid = None
        if lens is not None:       # abs_length = lens * L16 in fp32, truncated (speaker_similarity.py:107-110)
            valid = (lens.detach().to(device=x.device, dtype=torch.float32) * x.shape[-1]).int()
        return self.embed_16k(x, valid, return_stages)

    __call__ = forward


@torch.no_grad()
def cosine(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Cosine similarity of the rows of `a` and `b` [B, D] fp32 (eps 1e-8, as torch.nn.functional.cosine_similarity): [B]."""
    if not torch.is_tensor(a) or not torch.is_tensor(b) or a.dim() != 2 or a.shape != b.shape or a.dtype != torch.float32 or b.dtype != torch.float32:
        raise ValueError("`a` and `b` must be [B, D] fp32 tensors of one shape")
    _host.need_cuda(a.is_cuda and b.is_cuda, "spksim", "embeddings")
    out = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    a, b = a.contiguous(), b.contiguous()
    with torch.cuda.device(a.device):
        rc = _native.lib().ac_spk_cosine(_native._ptr(a), _native._ptr(b), int(a.shape[0]), int(a.shape[1]), _native._ptr(out), _native._stream())
    _native.check(rc, None, "ac_spk_cosine")
    return out


@torch.no_grad()
def speaker_similarity(hyp_sig: torch.Tensor, ref_sig: torch.Tensor, sample_rate: int, encoder: SpeakerEncoder, lens: torch.Tensor = None) -> torch.Tensor:
    """The cosine of the x-vectors of `hyp_sig` and `ref_sig` [B, T] (both at `sample_rate`): [B].  Hypothesis and reference go through
    the encoder as one batch of 2 B clips, as speaker_similarity.py:89-120 does; `lens` [B] are the relative lengths of both."""
    _host.check_sample_rate(sample_rate)
    if not torch.is_tensor(hyp_sig) or not torch.is_tensor(ref_sig) or hyp_sig.dim() != 2 or hyp_sig.shape != ref_sig.shape:
        raise ValueError("`hyp_sig` and `ref_sig` must be [B, T] tensors of the same shape")
    if not isinstance(encoder, SpeakerEncoder) or not encoder.pool:
        raise ValueError("`encoder` must be a SpeakerEncoder with pool=True")
    if hyp_sig.device != ref_sig.device:
        raise ValueError(f"`hyp_sig` is on {hyp_sig.device}, `ref_sig` on {ref_sig.device}")
    B = int(hyp_sig.shape[0])
    sig = torch.cat([hyp_sig.to(torch.float32), ref_sig.to(torch.float32)])
    embs = encoder.forward(sig, sample_rate, None if lens is None else torch.cat([lens, lens]))
    return cosine(embs[:B], embs[B:])


class SpkSimWavLM(_DistanceStats):
    """downstream/metrics/speaker_similarity.py:72-123: per clip the cosine similarity of the WavLM x-vectors of `hyp_sig` and `ref_sig`.
    `model` is a `SpeakerEncoder` (None: the checkpoint `model_hub`, fetched through transformers as the reference does).  Only the
    subset of ``MetricStats`` that `_DistanceStats` states exists."""

    __doc__ += _DistanceStats.__doc__

    def __init__(self, model_hub, sample_rate, save_path=None, model=None):
        self.sample_rate = sample_rate
        self.model = SpeakerEncoder(model_hub) if model is None else model
        self.clear()

    @torch.no_grad()
    def append(self, ids, hyp_sig, ref_sig, lens=None):
        if not torch.is_tensor(hyp_sig) or not torch.is_tensor(ref_sig) or hyp_sig.shape != ref_sig.shape or hyp_sig.dim() != 2:
            raise ValueError("`hyp_sig` and `ref_sig` must be [B, T] tensors of the same shape")
        self._record(ids, hyp_sig.shape[0], lambda: speaker_similarity(hyp_sig, ref_sig, self.sample_rate, self.model, lens))
