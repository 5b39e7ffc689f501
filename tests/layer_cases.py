"""Tap lists of the four codecs: the ONE place that maps the order in which `ac_debug_capture` emits module outputs to the
names of the oracle's layer lists (oracle/*_oracle.py `encoder_layers` / `decoder_layers` / `transformer_layers` / ...).

A `Tap` says, for one captured tensor: its name (also its key in the tiny fixtures), the oracle layer that produces it, its
layout, the tap its layer reads (`INPUT`: what the caller fed -- the signal, or the dequantised features), and, for a
captured tensor that is no layer of the path, why it is skipped.  `layer_fns` returns, per tap, a function from the input
tap's tensor to this tap's tensor, both in the oracle's layout of their tap, so that a test can run ONE layer on the
GPU's own previous output.  No GPU needed: tests/test_layer_cases.py checks the lists against the tiny fixtures on the CPU.

Layouts: the capture writes every tensor as [B][L][C].  "BCL" taps are [B,C,L] in the oracle (convs, LSTM, norms of the
vocoder backbone); "BTH" taps are [B,T,H] in the oracle too (Mimi's transformer layers: the capture's own layout).

`taps_of` lists what the capture emits, in order.  Six (codec, direction) pairs end in a layer that the capture does not emit
because it leaves through the call's RESULT: the last conv of EnCodec's and WavTokenizer's encoder (`sig_to_feats`) and the head
of every decoder (`toks_to_sig`).  `result_tap_of` names that layer -- a `Tap` with `result=True`: its oracle layer, the tap it
reads, and the layout of the call's return value -- and `layer_fns` holds its function too, so that a test can run it, like any
other layer, on the GPU's own last tap and compare with what the call returned.  Result layouts are those of the return value
itself: "BND" features [B,N,D] (the oracle's [B,D,N] with its last two axes exchanged), "BT" waveforms [B,T] (the oracle's
[B,1,T] without the channel axis; WavTokenizer's ISTFT head gives [B, N*hop] as it is).  DAC's and Mimi's encoders end in a
captured tap (`encoder.conv2`, `downsample`): they have no result layer."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

INPUT = "<input>"


@dataclass(frozen=True)
class Tap:
    name: str                    # capture order name == key of the tiny fixtures' activations
    oracle: Optional[str]        # name in the oracle's layer list (None for a skipped tap)
    layout: str                  # "BCL" or "BTH"
    src: str                     # the tap this layer reads, or INPUT
    skip: Optional[str] = None   # reason: captured, but compared by no layer test (its size is that of INPUT)
    result: bool = False         # not captured: the layer leaves through the call's return value; layout "BND" or "BT"


def _chain(names, oracle_names, layout="BCL", first_src=INPUT) -> List[Tap]:
    out, src = [], first_src
    for n, o in zip(names, oracle_names):
        out.append(Tap(n, o, layout, src))
        src = n
    return out


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


# ------------------------------------------------------------------------------------------------ EnCodec
def _seanet_enc_names(nr: int) -> List[str]:
    """enc0, then (resblock, down conv) per ratio, then the LSTM; the final conv is the call's result, not a tap."""
    names, i = ["enc0"], 1
    for _ in range(nr):
        names += [f"enc{i}", f"enc{i + 2}"]
        i += 3
    return names + [f"enc{i}"]


def encodec_taps(cfg, direction: str) -> List[Tap]:
    nr = len(_get(cfg, "upsampling_ratios"))
    if direction == "encode":
        names = _seanet_enc_names(nr)
    else:
        names, i = ["dec0", "dec1"], 2
        for _ in range(nr):
            names += [f"dec{i + 1}", f"dec{i + 2}"]
            i += 3
    return _chain(names, names)


# ------------------------------------------------------------------------------------------------ WavTokenizer
def wavtok_taps(cfg, direction: str) -> List[Tap]:
    if direction == "encode":
        names = _seanet_enc_names(len(cfg.ratios))
    else:
        names = ["embed", "pos0", "pos1", "pos2", "pos3", "pos4", "pos5", "norm"] + [f"cnx{l}" for l in range(cfg.num_layers)] + ["final"]
    return _chain(names, names)


# ------------------------------------------------------------------------------------------------ DAC
def dac_taps(cfg, direction: str) -> List[Tap]:
    if direction == "encode":
        nb = len(_get(cfg, "downsampling_ratios"))
        names = ["encoder.conv1"]
        for i in range(nb):
            names += [f"encoder.block.{i}.res_unit{u}" for u in (1, 2, 3)] + [f"encoder.block.{i}.conv1"]
        names.append("encoder.conv2")
        return _chain(names, names)
    nb = len(_get(cfg, "upsampling_ratios"))
    names = ["decoder.conv1"]
    for i in range(nb):
        names += [f"decoder.block.{i}.conv_t1"] + [f"decoder.block.{i}.res_unit{u}" for u in (1, 2, 3)]
    # the quantiser's output (from_codes) is captured first: it is the decoder's INPUT, not the output of one of its layers --
    # the codebook sums have their own tests (tests/test_codebook_search_gpu.py, toks_to_qfeats in the parity tests)
    skip = Tap("from_codes", None, "BCL", INPUT, "quantiser output: the decoder's input, not a decoder layer")
    return [skip] + _chain(names, names, first_src="from_codes")


# ------------------------------------------------------------------------------------------------ Mimi
def _mimi_short(oracle_name: str) -> str:
    """oracle tap name -> capture / fixture key: encoder.layers.3 -> enc3, decoder_transformer.layers.1 -> dectr1."""
    for long, short in (("encoder_transformer.layers.", "enctr"), ("decoder_transformer.layers.", "dectr"),
                        ("encoder.layers.", "enc"), ("decoder.layers.", "dec")):
        if oracle_name.startswith(long):
            return short + oracle_name[len(long):]
    return oracle_name


def mimi_taps(cfg, direction: str) -> List[Tap]:
    nr, nl = len(_get(cfg, "upsampling_ratios")), _get(cfg, "num_hidden_layers")
    if direction == "encode":
        o, i = ["encoder.layers.0"], 1
        for _ in range(nr):
            o += [f"encoder.layers.{i}", f"encoder.layers.{i + 2}"]
            i += 3
        o.append(f"encoder.layers.{i + 1}")
        conv = _chain([_mimi_short(n) for n in o], o)
        tr = [f"encoder_transformer.layers.{l}" for l in range(nl)]
        tf = _chain([_mimi_short(n) for n in tr], tr, "BTH", conv[-1].name)
        return conv + tf + [Tap("downsample", "downsample", "BCL", tf[-1].name)]
    # quantizer.decode is captured first ([B][N][hidden]): the decoder's INPUT, as DAC's from_codes
    skip = Tap("qdecode", None, "BCL", INPUT, "quantiser output: the decoder's input, not a decoder layer")
    up = Tap("upsample", "upsample", "BCL", "qdecode")
    tr = [f"decoder_transformer.layers.{l}" for l in range(nl)]
    tf = _chain([_mimi_short(n) for n in tr], tr, "BTH", "upsample")
    o, i = ["decoder.layers.0"], 1
    for _ in range(nr):
        o += [f"decoder.layers.{i + 1}", f"decoder.layers.{i + 2}"]
        i += 3
    # (decoder.layers.{i+1}, the head, is the call's result)
    return [skip, up] + tf + _chain([_mimi_short(n) for n in o], o, "BCL", tf[-1].name)


def _seanet_result(taps: List[Tap], direction: str) -> Tap:
    """EnCodec / WavTokenizer encoder: the final conv two module indices after the LSTM (the ELU between them has no entry);
    EnCodec decoder: the final conv two after the last residual block."""
    last = taps[-1].name
    name = f"{last[:3]}{int(last[3:]) + 2}"
    return Tap(name, name, "BND" if direction == "encode" else "BT", last, result=True)


def result_tap_of(codec: str, cfg, direction: str) -> Optional[Tap]:
    """The layer that leaves through the call's result (`sig_to_feats` when encoding, `toks_to_sig` when decoding), or None where
    the last layer of the direction is a captured tap.  It reads the LAST tap of `taps_of`."""
    assert direction in ("encode", "decode")
    taps = taps_of(codec, cfg, direction)
    if codec == "encodec":
        return _seanet_result(taps, direction)
    if codec == "wavtokenizer":
        return _seanet_result(taps, direction) if direction == "encode" else Tap("sig", "sig", "BT", taps[-1].name, result=True)
    if direction == "encode":
        return None
    if codec == "dac":
        return Tap("decoder.conv2", "decoder.conv2", "BT", taps[-1].name, result=True)
    o = taps[-1].oracle                                    # Mimi: decoder.layers.{i}, the last block -> the head two after it
    o = f"decoder.layers.{int(o.rsplit('.', 1)[1]) + 2}"
    return Tap(_mimi_short(o), o, "BT", taps[-1].name, result=True)


TAPS = {"encodec": encodec_taps, "wavtokenizer": wavtok_taps, "dac": dac_taps, "mimi": mimi_taps}


def taps_of(codec: str, cfg, direction: str) -> List[Tap]:
    assert direction in ("encode", "decode")
    return TAPS[codec](cfg, direction)


# ------------------------------------------------------------------------------------------------ oracle layer functions
def layer_fns(codec: str, cfg, W, direction: str) -> Dict[str, Callable]:
    """tap name -> fn(input tap's tensor, in the oracle layout of the INPUT tap) -> this tap's tensor in its own oracle
    layout, in the dtype of W.  Where a BTH layer reads a BCL tap or the reverse (Mimi: around the transformers) the
    transpose is added here.  INPUT is [B,1,T] samples (encode) or [B,hidden,N] dequantised features (decode).
    The result layer of `result_tap_of`, where there is one, comes last: its fn gives the call's return value, [B,N,D] or [B,T]."""
    if codec == "encodec":
        from oracle import encodec_oracle as O
        layers = dict(O.encoder_layers(cfg, W) if direction == "encode" else O.decoder_layers(cfg, W))
    elif codec == "wavtokenizer":
        from oracle import wavtokenizer_oracle as O
        layers = dict(O.encoder_layers(cfg, W) if direction == "encode" else O.decoder_layers(cfg, W))
    elif codec == "dac":
        from oracle import dac_oracle as O
        layers = dict(O.encoder_layers(cfg, W) if direction == "encode" else O.decoder_layers(cfg, W))
    else:
        from oracle import mimi_oracle as O
        if direction == "encode":
            layers = dict(O.encoder_layers(cfg, W) + O.transformer_layers(cfg, W, "encoder_transformer") + [O.downsample(cfg, W)])
        else:
            layers = dict([O.upsample(cfg, W)] + O.transformer_layers(cfg, W, "decoder_transformer") + O.decoder_layers(cfg, W))
    taps = taps_of(codec, cfg, direction)
    layout = {t.name: t.layout for t in taps}
    layout[INPUT] = "BCL"
    out = {}
    for t in taps:
        if t.skip:
            continue
        fn = layers[t.oracle]
        if layout[t.src] != t.layout:      # [B,C,L] <-> [B,T,H]
            fn = (lambda f: lambda x: f(x.transpose(1, 2)))(fn)
        out[t.name] = fn
    r = result_tap_of(codec, cfg, direction)
    if r is not None:
        assert layout[r.src] == "BCL" and r.name not in out
        fn = layers[r.oracle]
        if r.layout == "BND":                 # [B,D,N] -> [B,N,D]
            out[r.name] = (lambda f: lambda x: f(x).transpose(1, 2))(fn)
        elif r.oracle == "sig":               # the ISTFT head gives [B, N*hop] itself
            out[r.name] = fn
        else:                                 # [B,1,T] -> [B,T]
            out[r.name] = (lambda f: lambda x: f(x)[:, 0])(fn)
    return out


# ------------------------------------------------------------------------------------------------ capture <-> oracle layout
def to_oracle(tap: Tap, a):
    """captured [B,L,C] (array or tensor) -> the tap's oracle layout."""
    return a if tap.layout == "BTH" else (a.transpose(0, 2, 1) if isinstance(a, np.ndarray) else a.transpose(1, 2))


def split_capture(flat: np.ndarray, taps: List[Tap], shape_of: Callable[[Tap], tuple]) -> Dict[str, np.ndarray]:
    """Cut the captured floats into the taps' tensors, each in its ORACLE layout.  `shape_of(tap)` is the oracle-layout
    shape of the tap (for a skipped tap: of its tensor as [B,C,L]).  Asserts that the sizes sum to the capture size."""
    out, off = {}, 0
    for t in taps:
        shape = tuple(shape_of(t))
        n = int(np.prod(shape))
        assert off + n <= flat.size, (t.name, off, n, flat.size)
        a = flat[off : off + n]
        out[t.name] = a.reshape(shape) if t.layout == "BTH" else a.reshape(shape[0], shape[2], shape[1]).transpose(0, 2, 1)
        off += n
    assert off == flat.size, (off, flat.size)
    return out


# ------------------------------------------------------------------------------------------------ inputs of the isolation test
def gain_input(sig: torch.Tensor, which: str, burst: torch.Tensor) -> torch.Tensor:
    """Input A: the noise as drawn (golden_cases.noise: amplitude 0.1).  Input B, the range case of tests/test_split16_gpu.py in
    one batch: with three clips -- clip 0 x 1e-3, clip 1 x 1e-3 with 400 samples of `burst` x 30 added, clip 2 x 50; with
    two -- clip 0 quiet with the burst, clip 1 x 50; with one -- quiet with the burst."""
    if which == "A":
        return sig
    assert which == "B"
    s = sig.clone()
    B, T = s.shape
    b_clip = 1 if B >= 3 else 0
    s[: b_clip + 1] *= 1e-3
    t0 = min(9000, T // 3)
    s[b_clip, t0 : t0 + 400] += burst[:400] * 30.0
    s[b_clip + 1 :] *= 50.0
    return s
