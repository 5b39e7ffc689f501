"""Restatement of the Vocos decoder the reference's `Encodec(use_vocos=True)` calls (audiocodecs/encodec.py:53-66,130-138:
`vocos.codes_to_features(toks)` + `vocos.decode(feats, bandwidth_id=...)`, Vocos 0.1.0 as published).  PARITY UNPINNED: the
`vocos` package is not on disk, so this is pinned to the published modules, not to outputs of the reference.  The modules
themselves (`_adanorm`, `convnext`, `head`, `istft_same`) are oracle/wavtokenizer_oracle.py's, cross-checked against
transformers' Xcodec2 modules in tests/test_wavtok_oracle_golden.py; what is new here is their order (no pos_net) and
`codes_to_features`.  Everything runs in the dtype of the weights it is given (fp32: torch's own order; fp64: the gold)."""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F

from oracle.wavtokenizer_oracle import _adanorm, convnext, head

TABLES = "feature_extractor.codebook_weights"


def cast(sd: Dict[str, torch.Tensor], dtype=torch.float32) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()}


def codes_to_features(cfg, W, toks):
    """EncodecFeatures.get_encodec_codes' inverse as Vocos states it: toks [B,N,K] -> [B,N,input_channels], K from the tensor."""
    K = toks.shape[-1]
    assert 1 <= K <= W[TABLES].shape[0] // cfg.codebook_size
    offsets = torch.arange(K) * cfg.codebook_size
    return F.embedding(toks + offsets, W[TABLES]).sum(2)


def toks_to_sig(cfg, W, toks, bandwidth_id: int, taps: Optional[dict] = None):
    """toks [B,N,K] int64 -> [B, N*hop]; `taps` gets the module outputs `embed`, `norm`, `cnx{l}`, `final`, each [B,C,N]."""
    def tap(name, x):
        if taps is not None:
            taps[name] = x
        return x

    x = codes_to_features(cfg, W, toks).transpose(1, 2)                                   # [B, input_channels, N]
    x = tap("embed", F.conv1d(x, W["backbone.embed.weight"], W["backbone.embed.bias"], padding=3))
    x = tap("norm", _adanorm(x.transpose(1, 2), W, "backbone.norm", bandwidth_id).transpose(1, 2))
    for l in range(cfg.num_layers):
        x = tap(f"cnx{l}", convnext(x, W, f"backbone.convnext.{l}", bandwidth_id))
    x = tap("final", F.layer_norm(x.transpose(1, 2), (x.shape[1],), W["backbone.final_layer_norm.weight"],
                                  W["backbone.final_layer_norm.bias"], eps=1e-6).transpose(1, 2))
    return head(cfg, W, x.transpose(1, 2), taps)


def tap_names(cfg):
    return ["embed", "norm"] + [f"cnx{l}" for l in range(cfg.num_layers)] + ["final"]


def tokens(seed: int, B: int, N: int, K: int, vocab: int = 1024) -> torch.Tensor:
    return torch.randint(0, vocab, (B, N, K), generator=torch.Generator().manual_seed(seed))
