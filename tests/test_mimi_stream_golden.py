"""CPU checks of the streaming-encode fixture (tools/make_golden_mimi_stream.py) and of the streaming ABI's declarations.

transformers' streamed tokens must equal the fp32 oracle's batch tokens of the same signal wherever the fp64 margin clears TAU
(the oracle is causal: its tokens for the whole signal are those of every whole-frame prefix)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from mimi_stream_cases import CASES, HOP, make_signal, pushes
from oracle import mimi_oracle as O
from test_oracle_golden import tokens_match_up_to_ties

STREAM_SYMBOLS = {"ac_mimi_stream_state_bytes", "ac_mimi_stream_reset", "ac_mimi_stream_workspace_bytes", "ac_mimi_stream_encode"}


@pytest.fixture(scope="module")
def stream_golden():
    z = np.load(os.path.join(GOLDEN_DIR, "mimi_stream_golden.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


def test_fixture_schedules_and_shapes(stream_golden):
    z, meta = stream_golden
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "mimi_stream_golden.npz")) < 1 << 20
    for case in CASES:
        info = meta["cases"][case["name"]]
        assert info["pushes"] == pushes(case, info["frames"]) and sum(info["pushes"]) == info["frames"]
        shape = (info["B"], info["frames"], meta["K"])
        for part in ("stream", "oneshot", "margin"):
            assert z[f"{case['name']}_{part}"].shape == shape
        assert make_signal(case, GOLDEN_DIR).shape == (info["B"], info["frames"] * HOP)
        # the fixture says so when HF's streamed and one-shot tokens differ; on these cases they never do
        assert info["stream_vs_oneshot_differ"] == 0
        assert np.array_equal(z[f"{case['name']}_stream"], z[f"{case['name']}_oneshot"])
    assert max(meta["cases"]["tiny_long"]["frames"] * 2, 0) > 8192   # past the batch path's RoPE table


ORACLE_CASES = [c for c in CASES if c["cfg"] == "tiny"] + [c for c in CASES if c["name"] == "full_ragged"]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=[c["name"] for c in ORACLE_CASES])
def test_hf_stream_matches_oracle_batch(case, stream_golden, mimi_checkpoints):
    z, meta = stream_golden
    cfg, sd = mimi_checkpoints(case["cfg"], case["weights_seed"])
    sig = torch.from_numpy(make_signal(case, GOLDEN_DIR))
    with torch.no_grad():
        toks = O.sig_to_toks(cfg, O.cast_weights(sd, torch.float32), sig, None, meta["K"]).numpy()
    gold = z[f"{case['name']}_stream"].astype(np.int64)
    n, bad, excused = tokens_match_up_to_ties(toks, gold, z[f"{case['name']}_margin"])
    assert bad == 0 and n > 0.9 * gold.size, (n, bad, excused)


def test_header_and_exports_declare_the_stream_abi():
    from audiocodecs_amd import _native

    header = open(os.path.join(ROOT, "include", "audiocodecs_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(ac_[a-z_]+)\s*\(", header))
    assert STREAM_SYMBOLS <= declared
    assert STREAM_SYMBOLS <= set(_native.EXPORTS)
