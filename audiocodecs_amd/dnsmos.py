"""DNSMOS (P.808): the one neural metric of the reference's evaluation recipe whose weights ship with it (the reference's
downstream/metrics/dnsmos.py; downstream/test_sr.py:102-142), as one call on the device.

``dnsmos(sig, sample_rate, weights)`` resamples to 16 kHz (``audiocodecs_amd.resample``), cuts every clip into the 9.01 s windows the
reference scores (``dnsmos_segments``: the doubling of a short clip, the hop of one second and the windows its float arithmetic silently
skips, restated), computes librosa's log-mel features of every window and runs the fixed P.808 net over them -- five 3 x 3 convolutions,
three 2 x 2 max pools, a global maximum and three dense layers -- and returns the mean over a clip's windows.  It runs in the HIP library
(``ac_dnsmos``): the DFT and the four 32-channel convolutions are split16 MFMA GEMMs, the dB rule is applied as the
first convolution loads, pools and the global maximum run in the epilogues; there is no CPU fallback.  ``dnsmos_net`` is the net alone on
features of any size from 8 x 8 up.

The weights are data and not part of this package: ``load_weights(path)`` reads the ``.npz`` that tools/make_dnsmos_golden.py writes
(tests/golden/dnsmos_p808.npz) or a caller's own ``.onnx`` of the P.808 model.  The ONNX file is read by the small protobuf wire reader
below and accepted only if its node list is exactly the chain this module states; nothing of the graph is executed.

Only the reference's defaults are compiled: 16 kHz, n_fft 321, hop 160, periodic Hann, center = True with zero padding (librosa >= 0.10),
power 2, 120 Slaney mel filters over 0 .. 8000 Hz with Slaney norm, ``(power_to_db(S, ref=np.max) + 40) / 40`` with top_db = 80.

**Parity with librosa's melspectrogram / power_to_db and with onnxruntime is unpinned**: neither is on disk.  The front end is restated
from librosa's published algorithm and the net from the operators' definitions (tests/dnsmos_ref.py is that statement in fp64); the STFT
is pinned to ``torch.stft``, the filterbank to ``transformers.audio_utils.mel_filter_bank``, the net to ``torch.nn.functional.conv2d`` /
``max_pool2d`` and the window plan to a literal restatement of the reference's loop.
"""

from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from . import _metric_host as _host
from . import _native
from ._metric_host import SAMPLE_RATE
from .metrics import _DistanceStats

__all__ = ["dnsmos", "dnsmos_net", "dnsmos_segments", "load_weights", "read_onnx", "weights_from_onnx", "DnsmosWeights", "DNSMOS", "SAMPLE_RATE", "INPUT_LENGTH",
           "WINDOW", "FRAMES", "N_MELS", "WEIGHT_SHAPES"]

INPUT_LENGTH = 9.01
WINDOW = int(INPUT_LENGTH * SAMPLE_RATE)      # 144160 samples make a window; its first 144000 feed the features
FRAMES = 900
N_MELS = 120

# the 16 tensors, in the order of the library's flat array (include/audiocodecs_amd.h ac_dnsmos_weights_count)
WEIGHT_SHAPES = {
    "conv5.w": (32, 1, 3, 3), "conv5.b": (32,), "conv6.w": (32, 32, 3, 3), "conv6.b": (32,), "conv7.w": (32, 32, 3, 3), "conv7.b": (32,),
    "conv8.w": (32, 32, 3, 3), "conv8.b": (32,), "conv9.w": (64, 32, 3, 3), "conv9.b": (64,),
    "dense3.w": (64, 64), "dense3.b": (64,), "dense4.w": (64, 64), "dense4.b": (64,), "dense5.w": (64, 1), "dense5.b": (1,),
}

# the chain: (op type, the attributes that must hold where present)
_CONV = ("Conv", {"kernel_shape": [3, 3], "pads": [1, 1, 1, 1], "strides": [1, 1], "dilations": [1, 1], "group": 1, "auto_pad": ("NOTSET",)})
_POOL = ("MaxPool", {"kernel_shape": [2, 2], "strides": [2, 2], "pads": [0, 0, 0, 0], "ceil_mode": 0, "dilations": [1, 1], "auto_pad": ("NOTSET", "VALID")})
_RELU = ("Relu", {})
CHAIN = (("Unsqueeze", {"axes": [3]}), ("Transpose", {"perm": [0, 3, 1, 2]}),
         _CONV, _RELU, _POOL, _CONV, _RELU, _POOL, _CONV, _RELU, _CONV, _RELU, _POOL, _CONV, _RELU,
         ("Transpose", {"perm": [0, 2, 3, 1]}), ("ReduceMax", {"axes": [1, 2], "keepdims": 0}),
         ("MatMul", {}), ("Add", {}), _RELU, ("MatMul", {}), ("Add", {}), _RELU, ("MatMul", {}), ("Add", {}))
_REQUIRED = {"Conv": ("kernel_shape", "pads", "strides"), "MaxPool": ("kernel_shape", "strides"), "Unsqueeze": ("axes",), "Transpose": ("perm",), "ReduceMax": ("axes",)}


# ---- the protobuf wire format, as far as an ONNX file of this model needs it ---------------------------------------------------------
def _varint(buf, i):
    v = s = 0
    while True:
        if i >= len(buf):
            raise ValueError("truncated varint")
        b = buf[i]
        i += 1
        v |= (b & 0x7F) << s
        if b < 0x80:
            return v, i
        s += 7
        if s > 63:
            raise ValueError("varint longer than 64 bits")


def _fields(buf):
    """(field number, wire type, value) of every field of one message: an int for varints, a memoryview for the others."""
    buf = memoryview(buf)
    i, n = 0, len(buf)
    while i < n:
        key, i = _varint(buf, i)
        field, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt in (1, 5):
            w = 8 if wt == 1 else 4
            v, i = buf[i:i + w], i + w
        elif wt == 2:
            ln, i = _varint(buf, i)
            v, i = buf[i:i + ln], i + ln
        else:
            raise ValueError(f"wire type {wt} (field {field}) is not read")
        if i > n:
            raise ValueError("truncated message")
        yield field, wt, v


def _ints(wt, v, out):
    """A repeated int64 field, packed or not."""
    if wt == 0:
        out.append(v)
    else:
        j = 0
        while j < len(v):
            q, j = _varint(v, j)
            out.append(q)


def _signed(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def _tensor(buf):
    """TensorProto: dims = 1, data_type = 2, float_data = 4, name = 8, raw_data = 9 -> (name, fp32 array)."""
    dims, name, dtype, floats, raw = [], None, None, [], None
    for f, wt, v in _fields(buf):
        if f == 1:
            _ints(wt, v, dims)
        elif f == 2:
            dtype = v
        elif f == 4:
            floats.append(np.frombuffer(v, dtype="<f4") if wt == 2 else np.frombuffer(v, dtype="<f4", count=1))
        elif f == 8:
            name = bytes(v).decode()
        elif f == 9:
            raw = bytes(v)
    if dtype != 1:
        raise ValueError(f"initializer {name!r} has data_type {dtype}: only FLOAT (1) is read")
    data = np.frombuffer(raw, dtype="<f4") if raw is not None else (np.concatenate(floats) if floats else np.zeros(0, np.float32))
    n = int(np.prod(dims)) if dims else 1
    if data.size != n:
        raise ValueError(f"initializer {name!r}: {data.size} values for dims {dims}")
    return name, np.array(data, dtype=np.float32).reshape(dims)


def _node(buf):
    """NodeProto: input = 1, output = 2, op_type = 4, attribute = 5 (AttributeProto: name = 1, i = 3, s = 4, ints = 8)."""
    d = {"inputs": [], "outputs": [], "op": None, "attrs": {}}
    for f, wt, v in _fields(buf):
        if f == 1:
            d["inputs"].append(bytes(v).decode())
        elif f == 2:
            d["outputs"].append(bytes(v).decode())
        elif f == 4:
            d["op"] = bytes(v).decode()
        elif f == 5:
            name, ints, i = None, [], None
            for g, w2, u in _fields(v):
                if g == 1:
                    name = bytes(u).decode()
                elif g == 3:
                    i = _signed(u)
                elif g == 4:
                    i = bytes(u).decode()
                elif g == 8:
                    _ints(w2, u, ints)
            d["attrs"][name] = [_signed(q) for q in ints] if ints else i
    return d


def read_onnx(data: bytes):
    """(nodes, initializers) of an ONNX ModelProto (graph = 7; GraphProto: node = 1, initializer = 5): nodes are dicts with `op`, `inputs`,
    `outputs` and the integer attributes `attrs`; initializers map a name to an fp32 array."""
    graphs = [v for f, wt, v in _fields(data) if f == 7 and wt == 2]
    if len(graphs) != 1:
        raise ValueError("not an ONNX model: no graph field")
    nodes, tensors = [], {}
    for f, wt, v in _fields(graphs[0]):
        if f == 1 and wt == 2:
            nodes.append(_node(v))
        elif f == 5 and wt == 2:
            name, arr = _tensor(v)
            tensors[name] = arr
    return nodes, tensors


def weights_from_onnx(data: bytes) -> Dict[str, np.ndarray]:
    """The 16 tensors of a P.808 ONNX file under their short names.  Refuses a graph whose node list is not exactly `CHAIN`."""
    nodes, tensors = read_onnx(data)
    ops = [n["op"] for n in nodes]
    if ops != [c[0] for c in CHAIN]:
        raise ValueError(f"the graph is not the P.808 chain this module states: its nodes are {ops}")
    for k, (n, (op, want)) in enumerate(zip(nodes, CHAIN)):
        for key in _REQUIRED.get(op, ()):
            if n["attrs"].get(key) is None:
                raise ValueError(f"node {k} ({op}) has no `{key}`")
        for key, val in want.items():
            got = n["attrs"].get(key)
            if got is not None and (got not in val if isinstance(val, tuple) else got != val):
                raise ValueError(f"node {k} ({op}): {key} = {got}, the chain has {val}")
        if k and n["inputs"][0] != nodes[k - 1]["outputs"][0]:
            raise ValueError(f"node {k} ({op}) does not read node {k - 1}'s output: the graph is not a chain")
    out = {}
    convs = [n for n in nodes if n["op"] == "Conv"]
    for name, n in zip(("conv5", "conv6", "conv7", "conv8", "conv9"), convs):
        if len(n["inputs"]) != 3:
            raise ValueError(f"{name}: a Conv with a kernel and a bias is expected")
        out[name + ".w"], out[name + ".b"] = tensors[n["inputs"][1]], tensors[n["inputs"][2]]
    mms = [n for n in nodes if n["op"] == "MatMul"]
    adds = [n for n in nodes if n["op"] == "Add"]
    for name, m, a in zip(("dense3", "dense4", "dense5"), mms, adds):
        out[name + ".w"], out[name + ".b"] = tensors[m["inputs"][1]], tensors[a["inputs"][1]]
    _check_shapes(out)
    return out


def _check_shapes(w) -> None:
    for name, shape in WEIGHT_SHAPES.items():
        if name not in w:
            raise ValueError(f"the weights lack {name!r}")
        if tuple(w[name].shape) != shape:
            raise ValueError(f"{name} has shape {tuple(w[name].shape)}, the P.808 net has {shape}")


class DnsmosWeights:
    """The 16 fp32 tensors of the P.808 net (`tensors`: short name -> CPU tensor) and, per device, their packed image: built once on
    first use there, like `KnnIndex`."""

    def __init__(self, tensors):
        _check_shapes(tensors)
        self.tensors = {k: torch.as_tensor(np.asarray(tensors[k], dtype=np.float32)).contiguous() for k in WEIGHT_SHAPES}
        self._packed: Dict[int, torch.Tensor] = {}

    def flat(self) -> torch.Tensor:
        return torch.cat([self.tensors[k].reshape(-1) for k in WEIGHT_SHAPES])

    def packed(self, device: torch.device) -> torch.Tensor:
        idx = _host.device_index(device)
        if idx not in self._packed:
            L = _native.lib()
            flat = self.flat()
            if flat.numel() != L.ac_dnsmos_weights_count():
                raise _native.NativeError(f"the library expects {L.ac_dnsmos_weights_count()} weights, the package holds {flat.numel()}")
            nbytes = L.ac_dnsmos_packed_bytes()
            with torch.cuda.device(idx):
                dev = torch.device("cuda", idx)
                flat_dev = flat.to(dev)
                packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                rc = L.ac_dnsmos_pack(_native._ptr(flat_dev), flat.numel(), _native._ptr(packed), nbytes, _native._stream())
                _native.check(rc, None, "ac_dnsmos_pack")
                torch.cuda.current_stream().synchronize()      # (once per device: flat_dev may go, and other streams may use the image)
            self._packed[idx] = packed
        return self._packed[idx]


def load_weights(path) -> DnsmosWeights:
    """A `.npz` with the 16 short names (tools/make_dnsmos_golden.py writes tests/golden/dnsmos_p808.npz) or a P.808 `.onnx`."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"PK":
        with np.load(path) as z:
            return DnsmosWeights({k: z[k] for k in z.files})
    return DnsmosWeights(weights_from_onnx(data))


# ---- the host plan ----------------------------------------------------------------------------------------------------------------------
def dnsmos_segments(length_16k: int):
    """The first samples of the windows the reference scores in a clip of `length_16k` samples at 16 kHz (dnsmos.py:87-107), in its own
    float expressions: a clip shorter than int(9.01 * 16000) = 144160 is doubled until it is not (sample j of the result is x[j mod
    length]), num_hops = int(floor(len / 16000) - 9.01) + 1, window idx is audio[int(idx * 16000) : int((idx + 9.01) * 16000)] and is
    skipped when shorter than 144160 -- which int((idx + 9.01) * 16000) makes it for idx 7 .. 23.  Window 0 is always kept."""
    n = int(length_16k)
    if n < 1:
        raise ValueError(f"a clip of {n} samples has no window (the reference would double it forever)")
    fs = SAMPLE_RATE
    total = n
    while total < WINDOW:
        total *= 2
    num_hops = int(math.floor(total / fs) - INPUT_LENGTH) + 1
    starts = []
    for idx in range(num_hops):
        a, b = int(idx * fs), int((idx + INPUT_LENGTH) * fs)
        if min(b, total) - a < WINDOW:
            continue
        starts.append(a)
    return tuple(starts)


def _plan(lengths):
    """int32 [S * 4 + B * 2]: per window (clip, first sample, clip length, index in the clip), then per clip (first window, count)."""
    wins, clips = [], []
    for b, n in enumerate(lengths):
        starts = dnsmos_segments(n)
        clips += [len(wins) // 4, len(starts)]
        for i, s in enumerate(starts):
            wins += [b, s, n, i]
    return torch.tensor(wins + clips, dtype=torch.int32), len(wins) // 4, max(clips[1::2])


_PLANS: Dict[tuple, tuple] = {}      # (device, B, L16) -> the plan of a call without `lens`, on the device


def _weights(weights) -> DnsmosWeights:
    if isinstance(weights, DnsmosWeights):
        return weights
    if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__"):
        return load_weights(weights)
    raise ValueError("`weights` must be a DnsmosWeights or the path of a .npz / .onnx of the P.808 model (the weights are not part of this package: "
                     "tools/make_dnsmos_golden.py writes tests/golden/dnsmos_p808.npz)")


@torch.no_grad()
def dnsmos_net(feats: torch.Tensor, weights, return_layers: bool = False):
    """feats [S, H, W] (H = time, W = mel; H, W >= 8) -> the P.808 net's score [S] fp32.  With `return_layers` (score, layers, vec): the four
    feature maps the net stores, as [S, 32, h, w] views of channels-last memory (behind the first, second and fourth convolution's pool and
    behind the third convolution), and vec [S, 64], the global maxima behind the fifth."""
    weights = _weights(weights)
    if not torch.is_tensor(feats) or feats.dim() != 3:
        raise ValueError("`feats` must be a [S, H, W] tensor")
    S, H, W = (int(n) for n in feats.shape)
    if H < 8 or W < 8 or H > 4096 or W > 4096 or H * W > 1 << 22:
        raise ValueError(f"features of {H} x {W}: the net takes 8 <= H, W <= 4096 with H W <= 2^22")
    dev = feats.device
    sizes = [(H // 2, W // 2), (H // 4, W // 4), (H // 4, W // 4), (H // 8, W // 8)]
    if S == 0:
        score = torch.empty(0, dtype=torch.float32, device=dev)
        return (score, [torch.empty(0, 32, h, w, dtype=torch.float32, device=dev) for h, w in sizes], torch.empty(0, 64, dtype=torch.float32, device=dev)) if return_layers else score
    _host.need_cuda(feats.is_cuda, "dnsmos", "features")
    packed = weights.packed(dev)
    x = feats.detach().to(torch.float32).contiguous()
    score = torch.empty(S, dtype=torch.float32, device=dev)
    layers = [torch.empty(S, h, w, 32, dtype=torch.float32, device=dev) for h, w in sizes] if return_layers else [None] * 4
    vec = torch.empty(S, 64, dtype=torch.float32, device=dev) if return_layers else None
    ws = _host.sized_buffer("ac_dnsmos_workspace_bytes", dev, S=S, H=H, W=W)
    ptr = _native._ptr
    with torch.cuda.device(dev):
        rc = _native.lib().ac_dnsmos_net(ptr(x), S, H, W, ptr(packed), ptr(score), *(ptr(t) for t in layers), ptr(vec), ptr(ws), ws.numel(), _native._stream())
    _native.check(rc, None, "ac_dnsmos_net")
    if return_layers:
        return score, [t.permute(0, 3, 1, 2) for t in layers], vec
    return score


def _check_args(sig, sample_rate, lens):
    """Everything that can be refused without a GPU.  Returns (B, T, L16)."""
    _host.check_sample_rate(sample_rate)
    if not torch.is_tensor(sig) or sig.dim() != 2:
        raise ValueError("`sig` must be a [B, T] tensor")
    B, T = (int(n) for n in sig.shape)
    if lens is not None and (not torch.is_tensor(lens) or tuple(lens.shape) != (B,)):
        raise ValueError(f"`lens` must be a [B] tensor of relative lengths (B = {B})")
    L16 = _host.resampled_len(T, sample_rate)
    if L16 < 1:
        raise ValueError("a clip of 0 samples has no window (the reference would double it forever)")
    return B, T, L16


def _lengths(lens, B, L16):
    """Per clip int(lens[i] * L16): the product in float64 from the float32 value, as the reference's numpy expression; one host read."""
    if lens is None:
        return [L16] * B
    rel = lens.detach().to(torch.float32).cpu().numpy().astype(np.float64)
    out = []
    for i in range(B):
        n = min(int(rel[i] * L16), L16) if np.isfinite(rel[i]) else -1
        if n < 1:
            raise ValueError(f"clip {i} holds {max(n, 0)} samples after `lens` ({rel[i]}): it has no window (the reference would double it forever)")
        out.append(n)
    return out


@torch.no_grad()
def dnsmos(sig: torch.Tensor, sample_rate: int, weights, lens=None, return_segments: bool = False):
    """sig [B, T] at `sample_rate` -> the DNSMOS P.808 score [B] fp32 on the signal's device: the mean of the net's score over the windows
    `dnsmos_segments` keeps.  `lens` [B] (relative lengths, as the reference's `append`) cuts clip i to int(lens[i] * L16) samples at 16 kHz
    and costs one host read; without it the call reads nothing back and can be captured in a graph.  With `return_segments`
    (score, segments, feats): segments [B, Smax] the windows' scores, NaN past a clip's count; feats [S, 900, 120] the log-mel features
    of all windows, clip after clip.  A clip that holds an inf or a NaN scores NaN and disturbs no other clip."""
    from .resample import resample

    weights = _weights(weights)
    B, T, L16 = _check_args(sig, sample_rate, lens)
    dev = sig.device
    if B == 0:            # an empty shard: the empty result (the library is not called)
        score = torch.empty(0, dtype=torch.float32, device=dev)
        return (score, torch.empty(0, 0, dtype=torch.float32, device=dev), torch.empty(0, FRAMES, N_MELS, dtype=torch.float32, device=dev)) if return_segments else score
    lengths = _lengths(lens, B, L16)
    _host.need_cuda(sig.is_cuda, "dnsmos", "signal")
    x = resample(sig.detach().to(torch.float32), sample_rate, SAMPLE_RATE).contiguous()
    assert int(x.shape[1]) == L16
    key = (dev.index, B, L16)
    if lens is None and key in _PLANS:
        plan, S, Smax = _PLANS[key]
    else:
        plan, S, Smax = _plan(lengths)
        plan = plan.to(dev)
        if lens is None:
            if len(_PLANS) >= 64:
                _PLANS.clear()
            _PLANS[key] = (plan, S, Smax)
    tables, packed = _host.tables("dnsmos", dev), weights.packed(dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    segs = torch.empty(B, Smax, dtype=torch.float32, device=dev) if return_segments else None
    feats = torch.empty(S, FRAMES, N_MELS, dtype=torch.float32, device=dev) if return_segments else None
    ws = _host.sized_buffer("ac_dnsmos_workspace_bytes", dev, FRAMES, N_MELS, S=S)
    ptr = _native._ptr
    with torch.cuda.device(dev):
        rc = _native.lib().ac_dnsmos(ptr(x), B, L16, ptr(plan), S, Smax, ptr(tables), ptr(packed), ptr(score), ptr(segs), ptr(feats), ptr(ws), ws.numel(), _native._stream())
    _native.check(rc, None, "ac_dnsmos")
    return (score, segs, feats) if return_segments else score


class DNSMOS(_DistanceStats):
    """downstream/metrics/dnsmos.py: per clip the P.808 DNSMOS of `sig`.  `model` is a `DnsmosWeights` or the path of the weights; the
    reference's default (the ONNX file beside its source) does not exist here, so None is refused.  Only the subset of ``MetricStats`` that
    `_DistanceStats` states exists."""

    __doc__ += _DistanceStats.__doc__

    def __init__(self, sample_rate, model=None):
        if model is None:
            raise ValueError("DNSMOS needs `model`: a DnsmosWeights or the path of the P.808 weights -- the .npz that tools/make_dnsmos_golden.py writes "
                             "(tests/golden/dnsmos_p808.npz) or a model_v8.onnx; the weights are not part of this package")
        self.sample_rate = sample_rate
        self.model = _weights(model)
        self.clear()

    @torch.no_grad()
    def append(self, ids, sig, lens=None):
        """`lens` is honoured, as the reference honours it for this metric alone."""
        if not torch.is_tensor(sig) or sig.dim() != 2:
            raise ValueError("`sig` must be a [B, T] tensor")
        self._record(ids, sig.shape[0], lambda: dnsmos(sig, self.sample_rate, self.model, lens=lens))
