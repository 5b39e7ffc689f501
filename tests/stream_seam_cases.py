"""Segment geometry, case list and the per-element comparison for the stream-kernel seam tests (test_stream_seams_gpu.py; checked on
the CPU by test_stream_seam_cases.py).

The five stream kernels (csrc/stream_path.hip) cut a clip into SEGMENTS, one wave per segment; a kernel of that kind can only be subtly
wrong where a segment begins (warm-up chunk or tile, halo rows, padding at the clip start) or ends (short last segment, partial last
tile or chunk).  `geometry()` restates, in plain Python, how each launcher derives the segments from the batch size, the row count and the
developer switch; `seam_rows()` turns that into the tap rows at which a segment begins.

THE RESTATEMENT CAN DRIFT from stream_path.hip.  What guards it: the switch-forced cases of the GPU test must reproduce the default
geometry's taps bit for bit, every case asserts by `profile_kernels` that the kernel named here is the one that ran, and the comparison
itself is per element over the WHOLE tap -- the seam rows only label where the worst element sits, they select nothing.

What the launchers do, read from the code (stream_path.hip line numbers at the time of writing):
  * enc_stream (:172-175): chunks of 32 samples; seg_chunks = max(8, cdiv(nchunks, max(1, 4096 / B))), `front_seg` > 0 replaces it.
  * dec_stream (:219-222): chunks of 16 input rows (32 samples out); the same rule, `tail_seg` replaces it.
  * rb_stream6 (:21-25): tiles of 16 rows; seg_tiles = cdiv(tiles, min(tiles, max(1, 4096 / B))); `rb_stream` = n + 1 gives min(tiles, n).
  * rb_stream6m (:82-86): as rb_stream6 with a floor of 8 tiles in the HEAD form (a segment pays one warm-up tile); no switch.
  * rb_stream128m (:118-122): as rb_stream6 with 256 * WAVES / B, WAVES = 12 (EnCodec, 1x1 shortcut) or 16 (Mimi); no switch.
`min(tiles, want)` is the number of segments asked for, so a SMALL batch makes every 16-row tile a segment of its own (seam every 16 rows)
and only a batch above 4096 / tiles clips makes segments of two or more tiles, whose interior tiles take their halo from the tile before
instead of from memory.  Both regimes are in the case list.  In rb_stream128m `GRP = 4` groups the tiles of OUTPUT CHANNELS of one row
tile, not row tiles, so the row count does not meet it; the case list still holds row counts of 1, 2, 3 and 0 tiles modulo four.

Rows per tap (EnCodec, ratios 2, 4, 5, 8 from the sample rate down; N = cdiv(T, 320) frames): enc0 / enc1 T rows, enc3 / enc4 cdiv(T, 2),
enc6 / enc7 cdiv(T, 8); dec6 / dec7 40 N, dec9 / dec10 160 N, dec12 / dec13 / waveform 320 N.  The decoder's row counts are multiples of
8 (dec7) and of 16 (dec10, the input of dec_stream), and Mimi's last decoder block has 1920 N rows: dec_stream, the decoder's rb_stream6 and
rb_stream6m<head> never see a partial last tile, which test_stream_seam_cases.py asserts instead of pretending to cover it."""
from __future__ import annotations

import bisect
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from golden_cases import noise

# the project's per-element bar for module taps (test_gpu_parity.py::test_every_module_output_full_config_production_kernels)
ATOL, RTOL = 5e-6, 2e-5
# share of a case's tokens that fp64 near-tie frames may excuse (the suite as a whole sits at 2.2 %); cases under
# SMALL_CASE_TOKENS tokens instead allow at most one near-tie frame per clip
EXCUSED_CAP, SMALL_CASE_TOKENS = 0.05, 1000
RMS_BAR = 1e-5          # the whole-batch waveform bar of test_gpu_parity.py / test_shape_sweep_gpu.py / test_gpu_fullsize.py

KERNELS = ("enc_stream", "dec_stream", "rb_stream6", "rb_stream128m", "rb_stream6m_stem", "rb_stream6m_head")
UNIT = {"enc_stream": 32, "dec_stream": 16, "rb_stream6": 16, "rb_stream128m": 16, "rb_stream6m_stem": 16, "rb_stream6m_head": 16}
KNOB = {"enc_stream": "front_seg", "dec_stream": "tail_seg", "rb_stream6": "rb_stream"}      # ac_debug_set keys; the others have none
KNOB_DEFAULT = {"front_seg": 0, "tail_seg": 0, "rb_stream": 1}
ENC_FUSED_MIN_T = 64    # enc_front_ok (core.hip): below it the stem, rb_fused6<32> and thin_conv6 run as separate kernels


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def geometry(kernel: str, B: int, rows: int, knob: int = 0, waves: int = 16) -> Tuple[int, int, int]:
    """(unit, seg_units, nseg): rows per tile or chunk, tiles or chunks per segment, segments per clip.  `rows` is the kernel's INPUT
    row count (samples for enc_stream, the 64-channel rows for dec_stream); `knob` the value of KNOB[kernel] (0 / 1: default)."""
    unit = UNIT[kernel]
    units = cdiv(rows, unit)
    if kernel in ("enc_stream", "dec_stream"):
        seg = max(8, cdiv(units, max(1, 256 * 16 // B)))
        if knob > 0:
            seg = knob
        return unit, seg, cdiv(units, seg)
    want = max(1, 256 * (waves if kernel == "rb_stream128m" else 16) // max(1, B))
    if kernel == "rb_stream6" and knob > 1:
        seg = min(units, knob - 1)
    else:
        seg = cdiv(units, min(units, want))
        if kernel == "rb_stream6m_head":
            seg = max(8, seg)
    return unit, seg, cdiv(units, seg)


def last_segment_units(kernel: str, B: int, rows: int, knob: int = 0, waves: int = 16) -> int:
    unit, seg, nseg = geometry(kernel, B, rows, knob, waves)
    return cdiv(rows, unit) - (nseg - 1) * seg


def seam_rows(kernel: str, B: int, rows: int, knob: int = 0, waves: int = 16, scale=1) -> List[int]:
    """First row of every segment but the first, in tap rows: `scale` maps the kernel's input rows to the tap's rows (1/2 for enc3,
    2 for dec12 / dec13 / the waveform)."""
    unit, seg, nseg = geometry(kernel, B, rows, knob, waves)
    return [int(s * seg * unit * scale) for s in range(1, nseg)]


# ---- EnCodec: which kernel writes which tap, how many rows it has, and the rows its kernel cuts

ENC_TAPS = ["enc0", "enc1", "enc3", "enc4", "enc6", "enc7", "enc9", "enc10", "enc12", "enc13"]
DEC_TAPS = ["dec0", "dec1", "dec3", "dec4", "dec6", "dec7", "dec9", "dec10", "dec12", "dec13"]
TAP_KERNEL = {"enc0": "enc_stream", "enc1": "enc_stream", "enc3": "enc_stream", "enc4": "rb_stream6", "enc7": "rb_stream128m",
              "dec7": "rb_stream128m", "dec10": "rb_stream6", "dec12": "dec_stream", "dec13": "dec_stream", "wave": "dec_stream"}
ENCODEC_WAVES128 = 12
HOP = 320


def frames(T: int) -> int:
    return cdiv(T, HOP)


def tap_rows(tap: str, T: Optional[int] = None, N: Optional[int] = None) -> int:
    if tap.startswith("enc"):
        return {"enc0": T, "enc1": T, "enc3": cdiv(T, 2), "enc4": cdiv(T, 2), "enc6": cdiv(cdiv(T, 2), 4), "enc7": cdiv(cdiv(T, 2), 4),
                "enc9": cdiv(cdiv(cdiv(T, 2), 4), 5), "enc10": cdiv(cdiv(cdiv(T, 2), 4), 5), "enc12": frames(T), "enc13": frames(T)}[tap]
    N = frames(T) if N is None else N
    return {"dec0": N, "dec1": N, "dec3": 8 * N, "dec4": 8 * N, "dec6": 40 * N, "dec7": 40 * N, "dec9": 160 * N, "dec10": 160 * N,
            "dec12": 320 * N, "dec13": 320 * N, "wave": 320 * N}[tap]


def case_frames(case: dict) -> int:
    return case["N"] if "N" in case else frames(case["T"])


def tap_geometry(case: dict, tap: str, default: bool = False):
    """(kernel, input rows, knob, waves, scale) of a stream-kernel tap of an EnCodec case, or None for a tap no stream kernel writes."""
    kern = TAP_KERNEL.get(tap)
    if kern is None or (tap.startswith("enc") and ("T" not in case or case["T"] < ENC_FUSED_MIN_T and kern == "enc_stream")):
        return None
    knob = 0 if default else case.get("knobs", {}).get(KNOB.get(kern, ""), 0)
    if kern == "enc_stream":
        return kern, case["T"], knob, 16, (0.5 if tap == "enc3" else 1)
    if kern == "dec_stream":
        return kern, 160 * case_frames(case), knob, 16, 2
    rows = tap_rows(tap, case.get("T"), case.get("N"))
    return kern, rows, knob, ENCODEC_WAVES128, 1


def tap_seams(case: dict, tap: str, default: bool = False) -> List[int]:
    g = tap_geometry(case, tap, default)
    if g is None:
        return []
    kern, rows, knob, waves, scale = g
    return seam_rows(kern, case["B"], rows, knob, waves, scale)


# B, T (or N for a decode-only case), switches, ragged length, input seed.  Seeds were picked on the CPU so that the fp64 oracle's own
# near-ties stay inside EXCUSED_CAP (test_stream_seam_cases.py asserts it).
ENCODEC_CASES = [
    # batch-driven: segments of 4 tiles in enc4, of 2 tiles in enc7 / dec7 (55 tiles: the last segment is one tile), 28 segments of 8 chunks
    dict(name="b64_T7000", B=64, T=7000, seed=1),
    # batch-driven, decode only: dec7 60 tiles in segments of 2 and dec10 240 tiles in segments of 4, both with a full last segment
    dict(name="b64_N24_decode", B=64, N=24, seed=2),
    # switch-forced: 3 units per segment, 151 = 50 * 3 + 1 chunks / tiles (last segment: one unit, holding one row), 160 = 53 * 3 + 1
    dict(name="b3_T4801_seg3", B=3, T=4801, seed=1, knobs=dict(rb_stream=4, front_seg=3, tail_seg=3)),
    dict(name="b3_T4801_seg1", B=3, T=4801, seed=1, knobs=dict(rb_stream=2, front_seg=1, tail_seg=1)),
    # two tiles per segment at a small batch: the halo handed from tile to tile inside a segment (default there: every tile a segment)
    dict(name="b2_T2049_seg2", B=2, T=2049, seed=3, knobs=dict(rb_stream=3, front_seg=2, tail_seg=2)),
    # ragged: clip 1's mask edge (sample 1260) inside chunk 39, the warm-up chunk of the segment that begins at chunk 40
    dict(name="b4_T4803_ragged", B=4, T=4803, seed=4, length=[1.0, 1260.4 / 4803, 0.31, 0.003]),
    # the fused front's threshold and the fallback below it
    dict(name="b2_T63", B=2, T=63, seed=5),
    dict(name="b2_T64", B=2, T=64, seed=6),
    # last tile of enc7 with 15 rows (one tile) / 1 row (17 = 16 + 1) / 16 rows (48) / 15 rows (63: four tiles)
    dict(name="b2_T120", B=2, T=120, seed=7),
    dict(name="b2_T129", B=2, T=129, seed=8),
    dict(name="b2_T286", B=2, T=286, seed=9),      # enc4: 143 rows = 8 tiles + 15
    dict(name="b2_T303", B=2, T=303, seed=10),     # 15 / 16 / 17 samples in the last 32-sample chunk
    dict(name="b2_T304", B=2, T=304, seed=11),
    dict(name="b2_T305", B=2, T=305, seed=12),
    dict(name="b2_T382", B=2, T=382, seed=13),     # even / odd T below, at and above a chunk boundary (384 = 12 * 32)
    dict(name="b2_T383", B=2, T=383, seed=14),
    dict(name="b2_T384", B=2, T=384, seed=15),
    dict(name="b2_T385", B=2, T=385, seed=16),
    dict(name="b2_T386", B=2, T=386, seed=17),
    dict(name="b2_T503", B=2, T=503, seed=18),
    dict(name="b2_T1279", B=2, T=1279, seed=19),   # enc7: 160 rows = 10 tiles (2 modulo 4), full; enc4 640 rows
]


def encodec_case(name: str) -> dict:
    return next(c for c in ENCODEC_CASES if c["name"] == name)


def mask_edge(T: int, rel: float) -> int:
    """First zeroed sample: t >= T * length, the product in fp32 (as the kernel and the reference compare)."""
    return int(np.ceil(np.float32(T) * np.float32(rel)))


def case_input(case: dict) -> dict:
    if "T" in case:
        out = {"sig": noise(case["seed"], case["B"], case["T"])}
        if "length" in case:
            out["length"] = torch.tensor(case["length"], dtype=torch.float32)
        return out
    g = torch.Generator().manual_seed(case["seed"])
    return {"toks": torch.randint(0, 1024, (case["B"], case["N"], 8), generator=g)}


def capture_floats(case: dict) -> int:
    """Floats the capture hook writes for the larger of the two directions (every tap is [B][rows][C])."""
    chans = {"0": 32, "1": 32, "3": 64, "4": 64, "6": 128, "7": 128, "9": 256, "10": 256, "12": 512, "13": 512}
    enc = sum(tap_rows(t, case["T"]) * chans[t[3:]] for t in ENC_TAPS) if "T" in case else 0
    dchan = {"0": 512, "1": 512, "3": 256, "4": 256, "6": 128, "7": 128, "9": 64, "10": 64, "12": 32, "13": 32}
    dec = sum(tap_rows(t, case.get("T"), case.get("N")) * dchan[t[3:]] for t in DEC_TAPS)
    return case["B"] * max(enc, dec) + 4096


@functools.lru_cache(maxsize=None)
def _encodec_weights(dtype_name: str):
    from audiocodecs_amd import checkpoint
    from audiocodecs_amd.config import ENCODEC_24KHZ
    from oracle import encodec_oracle as O

    sd = checkpoint.synthetic_state_dict(ENCODEC_24KHZ, seed=0)
    return ENCODEC_24KHZ, O.fold_weight_norm(sd, getattr(torch, dtype_name))


def encodec_reference(case: dict, dtype=torch.float64, taps: bool = True) -> dict:
    """The oracle's answer for a case in `dtype`: tokens [B,N,K] and margins (encode cases), every module tap [B,C,rows] of the encoder
    and of the decoder run on those tokens, and the waveform as the tap "wave" [B,rows]."""
    from oracle import encodec_oracle as O

    cfg, W = _encodec_weights(str(dtype).split(".")[1])
    inp = case_input(case)
    out: Dict[str, object] = {}
    with torch.no_grad():
        if "sig" in inp:
            sig = inp["sig"].to(dtype)
            length = inp["length"].to(dtype) if "length" in inp else None
            out["toks"], out["margin"] = O.sig_to_toks(cfg, W, sig, length, 8, True)
            if taps:
                et: dict = {}
                O.masked_embeddings(cfg, W, sig, length, taps=et)
                out["enc"] = {k: v.numpy() for k, v in et.items()}
        else:
            out["toks"] = inp["toks"]
    return out


def encodec_decode_reference(toks: torch.Tensor, dtype=torch.float64) -> dict:
    from oracle import encodec_oracle as O

    cfg, W = _encodec_weights(str(dtype).split(".")[1])
    dt: dict = {}
    with torch.no_grad():
        wave = O.toks_to_sig(cfg, W, toks, taps=dt)
    taps = {k: v.numpy() for k, v in dt.items()}
    taps["wave"] = wave.numpy()
    return taps


# ---- Mimi: rb_stream6m<stem> and rb_stream128m<16> behind sig_to_feats, rb_stream6m<head> behind toks_to_sig

MIMI_HOP = 1920
# Mimi's features and waveform pass through a transformer, so the tap bar is not taken over as it stands.  Measured on the CPU over the
# cases below: the fp32 Mimi oracle lies within MIMI_FP32_DEV_FEATS * max(1, amax) of the fp64 one per feature element (largest:
# 1.10e-6 at 64 x 4321).  The EnCodec tap bar ATOL stands 5e-6 / 8.4e-7 = 5.95 times above the EnCodec fp32 oracle's measured deviation
# (ENCODEC_FP32_DEV); the kernel gets the same factor over the Mimi fp32 oracle: 6.61e-6 * max(1, amax) + RTOL * |ref|.
ENCODEC_FP32_DEV = 8.4e-7
MIMI_FP32_DEV_FEATS = 1.11e-6
MIMI_FEATS_ATOL = MIMI_FP32_DEV_FEATS * ATOL / ENCODEC_FP32_DEV
MIMI_ENC_CASES = [
    dict(name="mimi_b64_T4321", B=64, T=4321, seed=37),     # stem 271 tiles in segments of 5 (last: 1); 128-ch block 68 tiles in segments of 2
    dict(name="mimi_b32_T3840", B=32, T=3840, seed=32),     # stem 240 tiles in segments of 2
    dict(name="mimi_b2_T1919", B=2, T=1919, seed=33),
    dict(name="mimi_b2_T1920", B=2, T=1920, seed=34),
    dict(name="mimi_b2_T1921", B=2, T=1921, seed=35),
    dict(name="mimi_b2_T2044", B=2, T=2044, seed=37),       # 128-ch block: 511 rows = 31 tiles + 15
    dict(name="mimi_b3_T3841", B=3, T=3841, seed=45),
]
MIMI_DEC_CASES = [
    dict(name="mimi_b64_N5_decode", B=64, N=5, seed=41),    # 600 tiles, segments of 10: the 8-tile floor inactive
    dict(name="mimi_b3_N2_decode", B=3, N=2, seed=42),      # 240 tiles, floor active: 30 segments, 29 warm-up tiles
    dict(name="mimi_b1_N1_decode", B=1, N=1, seed=43),      # 120 tiles, 15 segments
    dict(name="mimi_b35_N10_decode", B=35, N=10, seed=44),  # 1200 tiles = 109 segments of 11 + 1: a last segment of one tile
]


def mimi_frames(T: int) -> int:
    return cdiv(T, MIMI_HOP)


def mimi_geometry(case: dict) -> Dict[str, Tuple[str, int]]:
    """kernel -> (geometry kernel name, input rows) for a Mimi case."""
    if "T" in case:
        return {"rb_stream6m_stem": ("rb_stream6m_stem", case["T"]), "rb_stream128m": ("rb_stream128m", cdiv(case["T"], 4))}
    return {"rb_stream6m_head": ("rb_stream6m_head", MIMI_HOP * case["N"]), "rb_stream128m": ("rb_stream128m", MIMI_HOP * case["N"] // 4)}


def mimi_case_input(case: dict) -> dict:
    if "T" in case:
        return {"sig": noise(case["seed"], case["B"], case["T"])}
    g = torch.Generator().manual_seed(case["seed"])
    return {"toks": torch.randint(0, 2048, (case["B"], case["N"], 8), generator=g)}


@functools.lru_cache(maxsize=None)
def _mimi_weights(dtype_name: str):
    from audiocodecs_amd import checkpoint
    from audiocodecs_amd.config import MIMI_24KHZ
    from oracle import mimi_oracle as O

    sd = checkpoint.synthetic_mimi_state_dict(MIMI_24KHZ, seed=0)
    return MIMI_24KHZ, O.cast_weights(sd, getattr(torch, dtype_name))


def mimi_reference(case: dict, dtype=torch.float64) -> dict:
    """Encode case: feats [B,N,H], tokens, margins and the taps of the first residual blocks (encoder.layers.1: 64 channels,
    encoder.layers.4: 128 channels) as [B,C,rows].  Decode case: the waveform [B,rows]."""
    from oracle import mimi_oracle as O

    cfg, W = _mimi_weights(str(dtype).split(".")[1])
    inp = mimi_case_input(case)
    with torch.no_grad():
        if "sig" in inp:
            sig = inp["sig"].to(dtype)
            taps: dict = {}
            z = O.embeddings(cfg, W, sig, taps)
            codes, m = O.rvq_encode(cfg, W, z, 8, True)
            return {"feats": z.movedim(-1, -2).numpy(), "toks": codes.permute(1, 2, 0).contiguous().numpy(),
                    "margin": m.permute(1, 2, 0).contiguous().numpy(),
                    "taps": {k: taps[k].numpy() for k in ("encoder.layers.0", "encoder.layers.1", "encoder.layers.3", "encoder.layers.4")}}
        return {"wave": O.toks_to_sig(cfg, W, inp["toks"]).numpy()}


# ---- the comparison

def worst(got, ref64, seams: Sequence[int] = (), atol: float = ATOL, rtol: float = RTOL) -> dict:
    """Largest |got - ref| / (atol * max(1, amax|ref|) + rtol * |ref|) over every element of a tap ([B,C,rows] or [B,rows], rows last)
    and where it sits: clip, channel, row, the segment the row is in and its distance to the nearest seam (None without seams).
    A value of 1 is the bar; a non-finite element counts as infinite."""
    ref = np.asarray(ref64, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    amax = float(np.abs(ref).max()) if ref.size else 0.0
    norm = np.abs(got - ref) / (atol * max(1.0, amax) + rtol * np.abs(ref))
    norm = np.where(np.isfinite(norm), norm, np.inf)
    if not norm.size:
        return dict(err=0.0, clip=None, channel=None, row=None, segment=None, seam_dist=None, amax=amax)
    idx = np.unravel_index(int(np.argmax(norm)), norm.shape)
    row = int(idx[-1])
    seams = sorted(seams)
    dist = min(abs(row - s) for s in seams) if seams else None
    return dict(err=float(norm[idx]), clip=int(idx[0]), channel=int(idx[1]) if norm.ndim == 3 else None, row=row,
                segment=bisect.bisect_right(seams, row), seam_dist=dist, amax=amax)


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.asarray(a, dtype=np.float64) ** 2)))


def near_tie_stats(margin, tau: float) -> Tuple[int, int, int]:
    """(tokens, tokens in near-tie frames -- what the margin policy excuses --, most near-tie frames in one clip)."""
    m = np.asarray(margin)
    safe = np.cumprod(m > tau, axis=-1).astype(bool)
    tie_frames = (~safe).any(axis=-1)
    return int(m.size), int((~safe).sum()), int(tie_frames.sum(axis=-1).max()) if m.size else 0


def excused_within_cap(margin, tau: float) -> bool:
    n, excused, per_clip = near_tie_stats(margin, tau)
    return per_clip <= 1 if n < SMALL_CASE_TOKENS else excused <= EXCUSED_CAP * n
