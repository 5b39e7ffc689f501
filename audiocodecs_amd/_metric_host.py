"""What the wrappers of the handle-free metrics share on the host (metrics.py, dnsmos.py, knn.py, tokstats.py):
the argument checks that several of them state in the same words, the refusal of a tensor that is not on a cuda device, the per-device
tables built from the library's fp64 source and the per-call workspace.  A metric's module keeps what is its own: its shapes, its
results and its call of the library."""

from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

from . import _native

SAMPLE_RATE = 16000   # what the signal metrics resample to
MAX_LEN = 1 << 24     # samples at 16 kHz a call takes
MAX_HYPS = 4          # hypotheses per call

_TABLES: Dict[Tuple[str, int], torch.Tensor] = {}


def check_sample_rate(sample_rate) -> None:
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate < 1:
        raise ValueError(f"`sample_rate` ({sample_rate!r}) must be a positive int")


def resampled_len(T: int, sample_rate: int) -> int:
    """The length of T samples at `sample_rate` once they stand at 16 kHz; refuses more than a call takes."""
    g = math.gcd(int(sample_rate), SAMPLE_RATE)
    L16 = int(math.ceil((SAMPLE_RATE // g) * T / (int(sample_rate) // g)))
    if L16 > MAX_LEN:
        raise ValueError(f"signals of {L16} samples at {SAMPLE_RATE} Hz are longer than the {MAX_LEN} a call takes: split them")
    return L16


def check_pair(hyp_sig, ref_sig, sample_rate):
    """`hyp_sig` [B, T] or [P, B, T] against `ref_sig` [B, T]: everything about the pair that can be refused without a GPU.  Returns
    (P or None, B, T, L16)."""
    check_sample_rate(sample_rate)
    if not torch.is_tensor(hyp_sig) or not torch.is_tensor(ref_sig):
        raise ValueError("`hyp_sig` and `ref_sig` must be tensors")
    if ref_sig.dim() != 2:
        raise ValueError(f"`ref_sig` must be [B, T] (got {tuple(ref_sig.shape)})")
    if hyp_sig.dim() not in (2, 3) or tuple(hyp_sig.shape[-2:]) != tuple(ref_sig.shape):
        raise ValueError(f"`hyp_sig` must be [B, T] or [P, B, T] with the shape of `ref_sig` {tuple(ref_sig.shape)} (got {tuple(hyp_sig.shape)})")
    P = int(hyp_sig.shape[0]) if hyp_sig.dim() == 3 else None
    if P is not None and not 1 <= P <= MAX_HYPS:
        raise ValueError(f"`hyp_sig` holds {P} hypotheses: a call takes 1..{MAX_HYPS}")
    B, T = (int(n) for n in ref_sig.shape)
    return P, B, T, resampled_len(T, sample_rate)


def need_cuda(on_cuda: bool, module: str, noun: str, clause: str = "move the {} to") -> None:
    """The one refusal of a CPU tensor: `module` is the metric's module, `noun` what the caller has to move."""
    if not on_cuda:
        raise _native.NativeError(f"audiocodecs_amd.{module} runs on MI355X only: {clause.format(noun)} a cuda device (there is deliberately no CPU fallback)")


def device_index(device: torch.device) -> int:
    return device.index if device.index is not None else torch.cuda.current_device()


def tables(name: str, device: torch.device) -> torch.Tensor:
    """The tables of metric `name` ("specdist", "stoi", "dnsmos"), built once per device from the library's fp64 source
    (ac_<name>_source on the host, one copy, ac_<name>_tables, one synchronise)."""
    idx = device_index(device)
    if (name, idx) not in _TABLES:
        L = _native.lib()
        n = getattr(L, f"ac_{name}_source_count")()
        src = torch.empty(n, dtype=torch.float64)
        _native.check(getattr(L, f"ac_{name}_source")(_native._ptr(src), n), None, f"ac_{name}_source")
        nbytes = getattr(L, f"ac_{name}_tables_bytes")()
        with torch.cuda.device(idx):
            src_dev = src.to(torch.device("cuda", idx))
            built = torch.empty(nbytes, dtype=torch.uint8, device=src_dev.device)
            _native.check(getattr(L, f"ac_{name}_tables")(_native._ptr(src_dev), _native._ptr(built), nbytes, _native._stream()), None, f"ac_{name}_tables")
            torch.cuda.current_stream().synchronize()      # (once per device: src_dev may go, and other streams may use the tables)
        _TABLES[name, idx] = built
    return _TABLES[name, idx]


def sized_buffer(query: str, device: torch.device, *unnamed, **shape) -> torch.Tensor:
    """The uint8 buffer of the size the library's `query` (an ac_*_bytes function) states for `shape` -- the arguments a refusal names,
    in the function's order -- followed by `unnamed`.  A size of 0 is the library's refusal of the shape."""
    nbytes = getattr(_native.lib(), query)(*shape.values(), *unnamed)
    if nbytes == 0:
        raise ValueError(f"{query} refuses " + ", ".join(f"{k}={v}" for k, v in shape.items()))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)
