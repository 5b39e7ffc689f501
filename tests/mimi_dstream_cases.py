"""Case lists for the streaming-decode tests (Mimi.decode_stream): which fixtures of tests/golden/mimi_golden.npz are decoded as
streams, and in which push schedules.  Tokens are the reference's own (`{name}.toks`), or the case's input tokens for the
decode-kind cases; the expected waveform is the reference's one-shot decode (`{name}.rec_strided`): the decoder is causal, so the
one-shot decode is the oracle of every push schedule (tests/test_mimi_dstream.py guards that)."""

from __future__ import annotations

import numpy as np
import torch

from mimi_cases import CASES, make_input
from mimi_stream_cases import pushes

NAMES = ["full_example", "full_noise_b2", "full_decode_rand", "full_decode_K1", "full_T4800_K32", "full_w1_noise", "tiny_taps", "tiny_odd"]
SCHEDULES = {"one_frame": [1], "ragged": [1, 2, 5, 1, 13, 4, 7, 1, 3]}


def case_of(name):
    return next(c for c in CASES if c["name"] == name)


def tokens_of(name, z, golden_dir) -> torch.Tensor:
    """[B, N, K] int64 (CPU)."""
    case = case_of(name)
    if case["kind"] == "decode":
        return make_input(case, golden_dir)["toks"].to(torch.int64)
    return torch.from_numpy(z[f"{name}.toks"].astype(np.int64))


def schedule(kind, frames):
    return pushes({"schedule": SCHEDULES[kind]}, frames)
