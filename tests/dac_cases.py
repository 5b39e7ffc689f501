"""Case list for the DAC golden fixtures (shared by tools/make_golden_dac.py and the tests).

The fixtures come from the STAND-IN (transformers.DacModel, same architecture) because the reference's
backend (descript-audio-codec) is not installed here: parity with the reference itself is unpinned
(oracle/dac_oracle.py header).  Inputs are re-drawn from the repo PRNG on both sides."""

from __future__ import annotations

import torch

from audiocodecs_amd import prng
from golden_cases import noise, tones

REC_STRIDE = 61

CASES = [
    # 44.1 kHz architecture (BASELINE.json configs[2]): strides (2,4,8,8), hop 512, 9 codebooks
    dict(name="full_noise_b2", cfg="full", weights_seed=0, kind="noise", B=2, T=22050, seed=211, K=9),
    dict(name="full_tones_K8", cfg="full", weights_seed=0, kind="tones", B=1, T=16000, seed=212, K=8),
    dict(name="full_T1023", cfg="full", weights_seed=0, kind="noise", B=1, T=1023, seed=213, K=9),  # 1 frame; T < 512 raises upstream
    dict(name="full_T512", cfg="full", weights_seed=0, kind="noise", B=2, T=512, seed=214, K=9),
    dict(name="full_T513", cfg="full", weights_seed=0, kind="noise", B=1, T=513, seed=215, K=9),
    dict(name="full_T4097_K1", cfg="full", weights_seed=0, kind="noise", B=1, T=4097, seed=216, K=1),
    dict(name="full_decode_rand", cfg="full", weights_seed=0, kind="decode", B=2, N=9, K=9, seed=221),
    dict(name="full_decode_K3", cfg="full", weights_seed=0, kind="decode", B=1, N=4, K=3, seed=222),
    dict(name="full_w1_noise", cfg="full", weights_seed=1, kind="noise", B=1, T=6000, seed=231, K=9),
    # tiny architecture (1/8 width, strides (2,4,5,8) incl. an odd one): every module output stored
    dict(name="tiny_taps", cfg="tiny", weights_seed=0, kind="noise", B=2, T=6400, seed=241, K=4, taps=True),
    dict(name="tiny_odd", cfg="tiny", weights_seed=0, kind="noise", B=3, T=3333, seed=242, K=3, taps=True),
]


def _rate_cases(tag: str, K: int, seed: int) -> list:
    """The cases of one published model other than the 44.1 kHz one: strides (2,4,5,8), hop 320, K codebooks.  T = 2049 gives 6 frames;
    T = 320 and T = 319 give one frame each (it decodes to 312 samples); K8 is the wrapper's default `num_codebooks`."""
    return [
        dict(name=f"{tag}_noise_b2", cfg=tag, weights_seed=0, kind="noise", B=2, T=2049, seed=seed, K=K, embs=True),
        dict(name=f"{tag}_T320", cfg=tag, weights_seed=0, kind="noise", B=1, T=320, seed=seed + 1, K=K),
        dict(name=f"{tag}_T319", cfg=tag, weights_seed=0, kind="noise", B=1, T=319, seed=seed + 2, K=K),
        dict(name=f"{tag}_tones_K8", cfg=tag, weights_seed=0, kind="tones", B=1, T=1601, seed=seed + 3, K=8),
        dict(name=f"{tag}_decode_rand", cfg=tag, weights_seed=0, kind="decode", B=2, N=5, K=K, seed=seed + 4),
    ]


# The 16 kHz and 24 kHz models (config.DAC_16KHZ: 12 codebooks, config.DAC_24KHZ: 32) at FULL width -- a list of its own, with a fixture
# file of its own (tests/golden/dac_rates_golden.npz, `tools/make_golden_dac.py --rates`): CASES is parametrised over the session's
# checkpoint fixture, which knows "full" and "tiny" only; the modules that use RATE_CASES build the two checkpoints themselves (rate_config).
RATE_CASES = _rate_cases("dac16", 12, 251) + _rate_cases("dac24", 32, 261)


def rate_config(tag: str):
    from audiocodecs_amd.config import DAC_16KHZ, DAC_24KHZ

    return {"dac16": DAC_16KHZ, "dac24": DAC_24KHZ}[tag]


_RATE_CKPT: dict = {}


def rate_checkpoint(tag: str):
    """tag -> (DacConfig, synthetic HF-layout state dict, seed 0); built once per process (about 10 s of CPU per config)."""
    if tag not in _RATE_CKPT:
        from audiocodecs_amd import checkpoint

        cfg = rate_config(tag)
        _RATE_CKPT[tag] = (cfg, checkpoint.synthetic_dac_state_dict(cfg, seed=0))
    return _RATE_CKPT[tag]


def make_input(case: dict, golden_dir: str) -> dict:
    kind = case["kind"]
    if kind == "noise":
        return {"sig": noise(case["seed"], case["B"], case["T"])}
    if kind == "tones":
        return {"sig": tones(case["seed"], case["B"], case["T"])}
    if kind == "decode":
        return {"toks": torch.from_numpy(prng.randint(case["seed"], "toks", (case["B"], case["N"], case["K"]), 1024))}
    raise ValueError(kind)
