"""Case lists for the streaming-EnCodec tests (Encodec.encode_stream / decode_stream): which fixtures of
tests/golden/encodec_golden.npz run as streams, over how many frames, and in which push schedules.  EnCodec is causal, so the
reference's one-shot result is the oracle of every push schedule once a stream has held back its first WARMUP frames
(tests/test_encodec_stream_oracle.py guards that)."""

from __future__ import annotations

import numpy as np
import torch

from golden_cases import CASES, make_input
from mimi_dstream_cases import SCHEDULES as _MIMI_SCHEDULES
from mimi_stream_cases import pushes

HOP = 320
WARMUP = 7      # max(kernel_size, last_kernel_size) of both configs; the tests check the stream objects derive the same
# encode cases: name -> whole frames streamed (full_tones_b2 has 37.5 frames of signal: its whole-frame prefix)
ENCODE_FRAMES = {"full_example": 793, "full_noise_b2": 75, "full_tones_b2": 37, "full_w1_noise": 15}
DECODE_ONLY = ["full_decode_rand", "full_decode_K16"]
SCHEDULES = dict(_MIMI_SCHEDULES, all_at_once=[1 << 30])     # frames per push, cycled (the stream itself holds back the warm-up)


def case_of(name):
    return next(c for c in CASES if c["name"] == name)


def schedule(kind, frames):
    return pushes({"schedule": SCHEDULES[kind]}, frames)


def signal_of(name, golden_dir) -> torch.Tensor:
    """[B, frames * HOP] float32 (CPU): the case's input cut to its whole frames."""
    return make_input(case_of(name), golden_dir)["sig"][:, : ENCODE_FRAMES[name] * HOP].contiguous()


def tokens_of(name, z, golden_dir) -> torch.Tensor:
    """[B, N, K] int64 (CPU): the reference's own tokens, or the input tokens of a decode-kind case."""
    case = case_of(name)
    if case["kind"] == "decode":
        return make_input(case, golden_dir)["toks"].to(torch.int64)
    return torch.from_numpy(z[f"{name}.toks"].astype(np.int64))
