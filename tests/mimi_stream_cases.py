"""Case list for the streaming-encode fixture (tests/golden/mimi_stream_golden.npz).

Shared by tools/make_golden_mimi_stream.py and the tests.  Inputs are re-drawn from the repo PRNG on both sides (as in
mimi_cases.py); the fixture stores only what transformers' MimiModel produced with OUR seeded synthetic weights.  A schedule
is a list of whole-frame push sizes (frames of hop = 1920 samples); it is cycled until `frames` frames have been pushed.
"""

from __future__ import annotations

import numpy as np

from golden_cases import noise, read_example_wav

HOP = 1920

CASES = [
    dict(name="tiny_b3_f40", cfg="tiny", weights_seed=0, B=3, frames=40, seed=301, schedule=[1]),
    # 4 160 frames = 8 320 transformer positions: past the 8 192-row RoPE table of the batch path
    dict(name="tiny_long", cfg="tiny", weights_seed=0, B=1, frames=4160, seed=302, schedule=[64]),
    dict(name="full_b2_f160", cfg="full", weights_seed=0, B=2, frames=160, seed=303, schedule=[3]),
    dict(name="full_ragged", cfg="full", weights_seed=0, B=1, frames=60, seed=304, schedule=[1, 2, 5, 1, 13, 4, 7, 1, 3]),
    dict(name="full_w1", cfg="full", weights_seed=1, B=2, frames=30, seed=305, schedule=[2, 1, 4]),
    dict(name="full_example", cfg="full", weights_seed=0, kind="wav", schedule=[1]),
]


def pushes(case, frames):
    """The case's schedule cycled (and the last push cut) to cover exactly `frames` frames."""
    out, done, i = [], 0, 0
    while done < frames:
        n = min(case["schedule"][i % len(case["schedule"])], frames - done)
        out.append(n)
        done += n
        i += 1
    return out


def make_signal(case, golden_dir) -> np.ndarray:
    """[B, frames*HOP] float32 (the example clip is cut to whole frames)."""
    if case.get("kind") == "wav":
        sig = read_example_wav(golden_dir).numpy()
        return np.ascontiguousarray(sig[:, : sig.shape[1] // HOP * HOP]).astype(np.float32)
    return noise(case["seed"], case["B"], case["frames"] * HOP).numpy().astype(np.float32)
