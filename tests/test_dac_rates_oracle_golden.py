"""Pins the DAC oracle (oracle/dac_oracle.py) at the 16 kHz and 24 kHz models -- config.DAC_16KHZ (12 codebooks) and
config.DAC_24KHZ (32), strides (2,4,5,8), full width -- to the STAND-IN fixtures of tests/golden/dac_rates_golden.npz
(`tools/make_golden_dac.py --rates`: transformers.DacModel holding the same synthetic weights, called as the wrapper calls dac.DAC).
The assertions are those of tests/test_dac_oracle_golden.py, unchanged; parity with the reference's own backend stays UNPINNED as it
is there.  The oracle is what tests/test_dac_rates_gpu.py holds the HIP path to on fresh inputs.  CPU-only."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from dac_cases import RATE_CASES, rate_checkpoint, rate_config
from oracle import dac_oracle as O
from test_dac_oracle_golden import check_oracle_case

_W = {}


@pytest.fixture(scope="module")
def rates_golden():
    z = np.load(os.path.join(GOLDEN_DIR, "dac_rates_golden.npz"))
    return z, json.loads(bytes(z["meta_json"]).decode())


# (decoding does not depend on the search variant: the decode-only cases run once)
PARAMS = [(c, v) for c in RATE_CASES for v in ("descript", "hf") if not (c["kind"] == "decode" and v == "hf")]


@pytest.mark.parametrize("case,variant", PARAMS, ids=[f"{c['name']}-{v}" for c, v in PARAMS])
def test_oracle_matches_standin_fixture(case, variant, rates_golden):
    z, meta = rates_golden
    tag = case["cfg"]
    if tag not in _W:
        cfg, sd = rate_checkpoint(tag)
        _W[tag] = (cfg, O.cast_weights(sd))
    check_oracle_case(case, variant, z, meta, *_W[tag])


def test_wrapper_picks_the_model_from_orig_sample_rate():
    """dac.py:55 of the reference: the model is chosen by int(orig_sample_rate / 1000), default 16 kHz.  The constructor alone: no
    handle, no GPU (tests/test_dac_rates_gpu.py runs what it picked)."""
    from audiocodecs_amd import DAC
    from audiocodecs_amd.config import DAC_16KHZ, DAC_24KHZ, DAC_44KHZ

    sd = {"encoder.conv1.weight": torch.zeros(1)}        # looked at when the handle is built, not before
    assert DAC(24000, state_dict=sd).config is DAC_16KHZ and DAC(24000, state_dict=sd).orig_sample_rate == 16000
    for orig, cfg in ((16000, DAC_16KHZ), (24000, DAC_24KHZ), (44100, DAC_44KHZ)):
        assert DAC(16000, orig, state_dict=sd).config is cfg and cfg.sampling_rate == orig
    with pytest.raises(ValueError, match="no DAC model for 48000 Hz"):
        DAC(48000, 48000, state_dict=sd)
    assert DAC(16000, state_dict=sd, num_codebooks=50)._K() == 12 and DAC(24000, 24000, state_dict=sd, num_codebooks=50)._K() == 32


def test_the_file_holds_every_case_and_stays_small(rates_golden):
    z, meta = rates_golden
    assert sorted(meta["cases"]) == sorted(c["name"] for c in RATE_CASES)
    for c in RATE_CASES:
        info, cfg = meta["cases"][c["name"]], rate_config(c["cfg"])
        assert info["K"] == c["K"] <= cfg.n_codebooks and info["toks_shape"][-1] == c["K"]
        if c["kind"] != "decode":
            assert info["toks_shape"] == [c["B"], cfg.num_frames(c["T"]), c["K"]]
            assert z[f"{c['name']}.margin64"].shape == tuple(info["toks_shape"])
        assert info["rec_shape"] == [c["B"], cfg.num_samples(info["toks_shape"][1])]
    for tag in ("dac16", "dac24"):      # one frame at T = 320 and at T = 319, decoding to 312 samples
        assert meta["cases"][f"{tag}_T320"]["rec_shape"] == meta["cases"][f"{tag}_T319"]["rec_shape"] == [1, 312]
        cfg = rate_config(tag)
        assert meta["cases"][f"{tag}_noise_b2"]["embs_shapes"] == [[cfg.n_codebooks, 1024, 8], [cfg.n_codebooks, 1024, cfg.hidden_size]]
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "dac_rates_golden.npz")) < 100_000
