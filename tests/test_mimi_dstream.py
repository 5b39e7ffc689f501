"""CPU side of streaming Mimi decode: the C ABI declares it, and the argument its GPU tests lean on holds -- the decoder is causal,
so the one-shot decode of a token sequence is the oracle of every way of pushing it."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT

SYMBOLS = ["ac_mimi_stream_decode_state_bytes", "ac_mimi_stream_decode_reset", "ac_mimi_stream_decode_workspace_bytes", "ac_mimi_stream_decode"]


def test_the_four_entry_points_are_declared_and_bound():
    from audiocodecs_amd import _native

    header = open(os.path.join(ROOT, "include", "audiocodecs_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ac_[a-z_]+)\s*\(", header))
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} is not declared in include/audiocodecs_amd.h"
        assert sym in _native.EXPORTS, f"{sym} is not in _native.EXPORTS"
    assert _native.EXPORTS["ac_mimi_stream_decode"] == _native.EXPORTS["ac_mimi_stream_encode"]      # same argument shape, mirrored
    assert _native.EXPORTS["ac_mimi_stream_decode_reset"] == _native.EXPORTS["ac_mimi_stream_reset"]


def test_the_wrapper_exports_the_stream_class():
    import audiocodecs_amd

    assert "MimiDecodeStream" in audiocodecs_amd.__all__
    assert hasattr(audiocodecs_amd.Mimi, "decode_stream")
    assert audiocodecs_amd.MimiDecodeStream.MAX_POSITIONS == audiocodecs_amd.MimiEncodeStream.MAX_POSITIONS


@pytest.mark.parametrize("cfg_name,N", [("tiny", 24), ("full", 16)])
def test_fp64_decode_of_a_prefix_is_the_prefix_of_the_decode(cfg_name, N, mimi_checkpoints):
    """toks_to_sig(toks[:, :n]) == toks_to_sig(toks)[:, :n * hop] in fp64 to 1e-12 absolute (measured: 6e-15 on a waveform of
    amplitude 2.7): no conv, attention row or up-sampler of the decoder looks ahead."""
    from audiocodecs_amd import prng
    from oracle import mimi_oracle as O

    cfg, sd = mimi_checkpoints(cfg_name, 0)
    W64 = O.cast_weights(sd, torch.float64)
    toks = torch.from_numpy(prng.randint(7001, "dstream_prefix", (2, N, 8), cfg.codebook_size)).to(torch.int64)
    hop = cfg.hop_length
    with torch.no_grad():
        whole = O.toks_to_sig(cfg, W64, toks)
        assert whole.dtype == torch.float64 and whole.shape == (2, N * hop)
        assert float(whole.abs().max()) > 1e-3
        for n in (1, 2, 7, N // 2):
            part = O.toks_to_sig(cfg, W64, toks[:, :n])
            err = float((part - whole[:, : n * hop]).abs().max())
            print(f"{cfg_name} n={n}: max |prefix decode - decode prefix| = {err:.3g}")
            assert err < 1e-12, (n, err)
