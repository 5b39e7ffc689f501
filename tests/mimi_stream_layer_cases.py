"""Cases of the streamed-Mimi sub-layer tests (tests/test_mimi_stream_layers_cpu.py, tests/test_mimi_stream_layers_gpu.py):
push schedules, signals, the fp32 oracle's activations and tokens of a signal, and the per-tap bar.

A schedule lists FRAMES per push; the transformers see `resample_stride` = 2 rows per frame.  With sliding_window = 250 the ring
holds R = 249 rows (tiny: window 6, R = 5)."""
import torch

from golden_cases import noise
from oracle import mimi_oracle as O

HOP = 1920
PARTS = {"encode": "encoder_transformer", "decode": "decoder_transformer"}

# Full config, lockstep, B = 1.  Rows per push 2, 4, 6, 116, 122, 260, 2, 248, 2, 10 at positions 0, 2, 6, 12, 128, 250, 510, 512,
# 760, 762: a partial block of four query waves; the first query that no longer sees position 0 as row 0 of a push (250); a push of
# T = 260 > R whose append would overwrite what its own queries read, and which fills the ring alone; T = R - 1 = 248; a ring
# wrapped three times; 3 key blocks of 64 and a remainder of 58 (the query at 249 sees 250 keys).
FULL_FRAMES = [1, 2, 3, 58, 61, 130, 1, 124, 1, 5]
# Tiny config (window 6, R = 5, head_dim 16, 4 heads), lockstep, B = 3: almost every push has T >= R.
TINY_FRAMES = [1, 1, 2, 3, 1, 4]
# Slot pushes, full config, capacity 3: slot 0 alone to position 300, then slot 2 opens; [2, 0] for 3 frames, [0, 2] for 2.
SLOT_ALONE_FRAMES = [100, 50]
SLOT_JOINT = [([2, 0], 3), ([0, 2], 2)]
# Stale ring, tiny config, capacity 2: slot 1 runs 4 + 4 rows (past the ring of 5), is closed and reopened, then runs these.
STALE_FIRST_FRAMES = [2, 2]
STALE_SECOND_FRAMES = [1, 2, 1]

SEED = {"full": 9401, "tiny": 9402, "slot0": 9403, "slot2": 9404, "stale0": 9405, "stale1": 9406}

# absolute positions named in a failure: the window edge of the full config
NAMED_POSITIONS = (0, 249, 250, 251)


def bar(ref64):
    """The project's per-tap bar (tests/test_layer_isolation_gpu.py `_judge`), elementwise."""
    return 5e-6 * max(1.0, float(ref64.abs().max())) + 2e-5 * ref64.abs()


def rows_of(frames, stride=2):
    return [f * stride for f in frames]


def starts_of(frames, stride=2):
    out, p = [], 0
    for f in frames:
        out.append(p)
        p += f * stride
    return out


def signal(seed, B, frames):
    return noise(seed, B, frames * HOP)


_ORACLE = {}


def oracle_run(key, cfg, W, sig, K=8):
    """The fp32 oracle on `sig` [B, frames*HOP], once per `key`: the encoder transformer's input "x_enc" [B,T,H] and the tokens
    "toks" [B,N,K]."""
    if key not in _ORACLE:
        with torch.no_grad():
            x = O.encoder(cfg, W, sig[:, None])
            y = O.transformer(cfg, W, x.transpose(1, 2), "encoder_transformer").transpose(1, 2)
            z = O.fold([O.downsample(cfg, W)], y, None)
            toks = O.rvq_encode(cfg, W, z, K).permute(1, 2, 0).contiguous()
        _ORACLE[key] = {"x_enc": x.transpose(1, 2).contiguous(), "toks": toks}
    return _ORACLE[key]


def split_rows(x, sizes):
    """x [B,T,...] -> the pushes of `sizes` rows (all of x)."""
    assert sum(sizes) == x.shape[1], (sum(sizes), tuple(x.shape))
    return list(torch.split(x, sizes, 1))
