"""Every layer of the FULL-size codecs on its own against fp64.

Arming `ac_debug_capture` makes one encode / decode call emit every module output in order (tests/layer_cases.py).  The GPU's
own tap k-1 is the exact input its kernel(s) for layer k saw, so  ref64 = layer_k(tap[k-1].double())  computed on the CPU from the
oracle's layer lists isolates that layer: nothing upstream spends the budget.  The bar is the per-tap bar of
tests/test_gpu_parity.py::test_every_module_output_full_config_production_kernels, unchanged,

    |got - ref64| <= 5e-6 * max(1, max|ref64|) + 2e-5 * |ref64|        elementwise,

now spent on ONE layer.  Per tap two figures are recorded (parity_record) and printed, and NOT asserted on:

    e_gpu = rms(got - ref64) / rms(ref64)        e_ref = rms(ref32 - ref64) / rms(ref64)

ref32 being the same layer of the fp32 oracle on the same input: e_gpu / e_ref is what "fp32-grade" means for that kernel
("Per-layer error against fp64").

Cases: each codec at its full config, synthetic weights seed 0, both precisions (None: split16, "fp32_exact"), input A (noise x 0.1)
and input B (the range case of tests/test_split16_gpu.py folded into one batch: layer_cases.gain_input), at the smallest sizes
that still reach the seams -- EnCodec B=3 T=24007 (76 frames, a ragged last tile, the LSTM ring wrapped 9 times), Mimi B=2
T=1920*6+7, DAC B=2 T=2049, WavTokenizer B=2 T=6001 -- plus one Mimi capture of 261 transformer rows (past sliding_window = 250
and past four 64-query tiles + 5 rows) of which only the transformer layers are recomputed.  Decoding takes the fp32 oracle's
tokens of the same signal.

What is NOT covered here, because the hook does not emit it: the last conv of EnCodec's / WavTokenizer's encoder and the head of
every decoder (they leave through the call's result).  What the hook changes in the route is listed in
`test_production_kernels_run_under_the_hook`."""
import re

import numpy as np
import pytest
import torch

import layer_cases as LC
import parity_record
from golden_cases import noise
from test_gpu_parity import capture

pytestmark = pytest.mark.gpu

SHAPES = {"encodec": (3, 24000 + 7), "mimi": (2, 1920 * 6 + 7), "dac": (2, 2049), "wavtokenizer": (2, 6000 + 1)}
SEEDS = {"encodec": 9301, "mimi": 9302, "dac": 9303, "wavtokenizer": 9304}
PRECISIONS = [None, "fp32_exact"]
MIMI_TF_ROWS = 261
NAMED_ROWS = (0, 63, 64, 249, 250, 251, 260)      # tile seams of the 64-query attention tiles and the window edge (sliding_window = 250)

_CACHE = {}


def _oracle(name):
    import importlib

    return importlib.import_module({"encodec": "oracle.encodec_oracle", "mimi": "oracle.mimi_oracle", "dac": "oracle.dac_oracle",
                                    "wavtokenizer": "oracle.wavtokenizer_oracle"}[name])


def _weights(name, request):
    """-> (cfg, state dict, W fp32, W fp64), once per module."""
    if ("W", name) not in _CACHE:
        fx = {"encodec": "checkpoints", "mimi": "mimi_checkpoints", "dac": "dac_checkpoints", "wavtokenizer": "wavtok_checkpoints"}[name]
        cfg, sd = request.getfixturevalue(fx)("full", 0)
        O = _oracle(name)
        cast = O.fold_weight_norm if name == "encodec" else O.cast_weights
        _CACHE["W", name] = (cfg, sd, cast(sd), cast(sd, torch.float64))
    return _CACHE["W", name]


def _codec(name, precision, request):
    if ("codec", name, precision) not in _CACHE:
        from audiocodecs_amd import DAC, Encodec, Mimi, WavTokenizer

        cfg, sd, _, _ = _weights(name, request)
        if name == "encodec":
            c = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg, precision=precision)
        elif name == "mimi":
            c = Mimi(24000, num_codebooks=8, state_dict=sd, config=cfg, precision=precision)
        elif name == "dac":
            c = DAC(44100, 44100, num_codebooks=9, state_dict=sd, config=cfg, precision=precision)
        else:
            c = WavTokenizer(24000, state_dict=sd, arch=cfg, precision=precision)
        c = c.eval()
        c.sig_to_toks(noise(1, 1, 4800).cuda())          # creates the native handle
        _CACHE["codec", name, precision] = c
    return _CACHE["codec", name, precision]


def _signal(name, which, B=None, T=None):
    b, t = SHAPES[name]
    B, T = B or b, T or t
    return LC.gain_input(noise(SEEDS[name], B, T), which, noise(SEEDS[name] + 50, 1, 400)[0])


def _oracle_tokens(name, which, request):
    """The fp32 oracle's tokens of the case's signal (shared by both precisions)."""
    if ("toks", name, which) not in _CACHE:
        cfg, sd, W, _ = _weights(name, request)
        O = _oracle(name)
        sig = _signal(name, which)
        with torch.no_grad():
            if name == "wavtokenizer":
                t = O.sig_to_toks(cfg, W, sig)
            elif name == "dac":
                t = O.sig_to_toks(cfg, W, sig, None, 9)
            else:
                t = O.sig_to_toks(cfg, W, sig, None, 8)
        _CACHE["toks", name, which] = t
    return _CACHE["toks", name, which]


def _dequantised(name, codec, cfg, W, toks):
    """The decoder's INPUT [B,hidden,N].  EnCodec / WavTokenizer: the GPU's own dequantised features (the hook does not emit them);
    Mimi / DAC: the hook emits them as the first, skipped tap -- only the SHAPE of this tensor is used there."""
    O = _oracle(name)
    with torch.no_grad():
        if name in ("encodec", "wavtokenizer"):
            return codec.toks_to_qfeats(toks.cuda()).cpu().transpose(1, 2).contiguous()
        if name == "mimi":
            return O.rvq_decode(cfg, W, toks.movedim(-1, -2))
        return O.from_codes(cfg, W, toks.movedim(-1, -2))[0]


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def _meta_shapes(name, cfg, W, direction, x_shape):
    """Oracle-layout shape of every tap from a dry run on the meta device (no arithmetic)."""
    Wm = {k: v.to("meta") for k, v in W.items()}
    fns = LC.layer_fns(name, cfg, Wm, direction)
    shapes = {LC.INPUT: tuple(x_shape)}
    layout = {LC.INPUT: "BCL"}
    for t in LC.taps_of(name, cfg, direction):
        layout[t.name] = t.layout
        s = shapes[t.src]
        if t.skip:
            shapes[t.name] = s
        elif t.layout == "BTH":      # a transformer layer keeps its [B,T,H]
            shapes[t.name] = s if layout[t.src] == "BTH" else (s[0], s[2], s[1])
        else:
            shapes[t.name] = tuple(fns[t.name](torch.empty(s, device="meta")).shape)
    return shapes


def isolate(name, cfg, W, W64, direction, flat, x0, case, only=None, named_rows=()):
    """Walk the capture `flat` of one call: per layer, fp64 and fp32 references from the GPU's own previous tap, the bar, the two
    figures.  `only(tap)`: recompute just these layers (the others' sizes come from a dry run).  Returns the failure messages."""
    taps = LC.taps_of(name, cfg, direction)
    f32, f64 = LC.layer_fns(name, cfg, W, direction), LC.layer_fns(name, cfg, W64, direction)
    shapes = _meta_shapes(name, cfg, W, direction, x0.shape) if only else None
    vals, off, failures, figures = {LC.INPUT: x0}, 0, [], {}
    for t in taps:
        check = not t.skip and (only is None or only(t))
        if check:
            x = vals[t.src]
            with torch.no_grad():
                ref64 = f64[t.name](x.double())
                ref32 = f32[t.name](x)
            shape = tuple(ref64.shape)
        else:
            shape = shapes[t.name] if shapes else tuple(vals[t.src].shape)      # (a skipped tap has the size of INPUT)
        n = int(np.prod(shape))
        assert off + n <= flat.size, f"{case}: the capture ends inside tap {t.name} ({off} + {n} > {flat.size})"
        got = torch.from_numpy(flat[off : off + n])
        got = got.view(shape) if t.layout == "BTH" else got.view(shape[0], shape[2], shape[1]).transpose(1, 2)
        off += n
        vals[t.name] = got
        if not check:
            continue
        err = (got.double() - ref64).abs()
        amax = float(ref64.abs().max())
        tol = 5e-6 * max(1.0, amax) + 2e-5 * ref64.abs()
        e_gpu, e_ref = _rms(got.double() - ref64) / max(_rms(ref64), 1e-300), _rms(ref32.double() - ref64) / max(_rms(ref64), 1e-300)
        figures[t.name] = {"e_gpu": e_gpu, "e_ref": e_ref, "ratio": e_gpu / max(e_ref, 1e-300), "worst_err_over_tol": float((err / tol).max())}
        print(f"{case} {direction} {t.name:>28}: e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  ratio {e_gpu / max(e_ref, 1e-300):6.2f}  "
              f"worst |err|/tol {float((err / tol).max()):.3f}  max|ref64| {amax:.3e}")
        bad = err > tol
        if not bool(torch.isfinite(got).all()) or bool(bad.any()):
            i = int((err / tol).flatten().argmax())
            idx = tuple(int(v) for v in np.unravel_index(i, err.shape))
            msg = (f"layer {t.name} ({direction}, {case}): {int(bad.sum())} of {bad.numel()} elements beyond the bar; worst at {idx}: "
                   f"got {float(got[idx]):.9g} ref64 {float(ref64[idx]):.9g} |err| {float(err[idx]):.3e} tol {float(tol[idx]):.3e}; max|ref64| {amax:.3e}")
            if named_rows:     # [B,T,H]: the seam rows by name
                msg += "; rows " + ", ".join(f"row {r}: worst |err|/tol {float((err[:, r] / tol[:, r]).max()):.3f}" for r in named_rows)
            failures.append(msg)
        elif named_rows:
            for r in named_rows:
                assert bool((err[:, r] <= tol[:, r]).all()), f"layer {t.name} ({case}): row {r}"
    assert off == flat.size, f"{case}: {flat.size - off} captured floats beyond the tap list"
    parity_record.record(name, f"layer_isolation/{case}/{direction}", per_layer=figures)
    return failures


def _run_case(name, precision, which, request):
    cfg, sd, W, W64 = _weights(name, request)
    codec = _codec(name, precision, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    case = f"{name}/{precision or 'split16'}/{which}"
    sig = _signal(name, which)
    _, flat = capture(codec, lambda: codec.sig_to_toks(sig.cuda()), 1 << 26)
    failures = isolate(name, cfg, W, W64, "encode", flat, sig[:, None], case)
    toks = _oracle_tokens(name, which, request)
    x0 = _dequantised(name, codec, cfg, W, toks)
    rec, flat = capture(codec, lambda: codec.toks_to_sig(toks.cuda()), 1 << 26)
    assert bool(torch.isfinite(rec).all())
    failures += isolate(name, cfg, W, W64, "decode", flat, x0, case)
    return failures


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("precision", PRECISIONS, ids=["split16", "fp32_exact"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_layer_alone_against_fp64(name, precision, which, request):
    failures = _run_case(name, precision, which, request)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("precision", PRECISIONS, ids=["split16", "fp32_exact"])
def test_mimi_transformer_layers_past_the_window_and_the_query_tiles(precision, request):
    """261 rows at 25 Hz: past sliding_window = 250 (rows 250.. no longer see row 0) and past four 64-query tiles with a 5-row
    remainder.  Only the enctr* / dectr* layers are recomputed; the SEANet layers of this 10 s clip are walked over by size."""
    cfg, sd, W, W64 = _weights("mimi", request)
    assert cfg.sliding_window == 250 and cfg.head_dim == 64
    codec = _codec("mimi", precision, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    T = 960 * MIMI_TF_ROWS
    sig = _signal("mimi", "A", 1, T)
    case = f"mimi/{precision or 'split16'}/tf{MIMI_TF_ROWS}"
    only = lambda t: t.layout == "BTH"
    toks, flat = capture(codec, lambda: codec.sig_to_toks(sig.cuda()), 1 << 27)
    assert toks.shape[1] == (MIMI_TF_ROWS + 1) // 2          # 131 frames: the decoder's transformer sees 262 rows
    failures = isolate("mimi", cfg, W, W64, "encode", flat, sig[:, None], case, only, NAMED_ROWS)
    toks = toks.cpu()
    with torch.no_grad():
        x0 = _oracle("mimi").rvq_decode(cfg, W, toks.movedim(-1, -2))
    _, flat = capture(codec, lambda: codec.toks_to_sig(toks.cuda()), 1 << 27)
    failures += isolate("mimi", cfg, W, W64, "decode", flat, x0, case, only, NAMED_ROWS)
    assert not failures, "\n".join(failures)


def _names_under_hook(codec, sig, toks, detail=False):
    from audiocodecs_amd._native import debug_set

    if detail:
        debug_set(codec, "prof_detail", 1)
    try:
        stats = codec.profile_kernels(lambda: (capture(codec, lambda: codec.sig_to_toks(sig), 1 << 26), capture(codec, lambda: codec.toks_to_sig(toks), 1 << 26)))
    finally:
        if detail:
            debug_set(codec, "prof_detail", 0)
    return {s[0] for s in stats}


@pytest.mark.parametrize("name", list(SHAPES))
def test_production_kernels_run_under_the_hook(name, request):
    """The layer tests above judge the kernels that run WITH the hook armed; this pins which those are (split16 precision, input A's
    shapes).  Where the hook changes the route the kernel it displaces is named here and checked to run without the hook:

      * EnCodec: the hook changes nothing -- enc_stream / dec_stream write the module outputs inside their chains themselves while
        it is armed (core.hip encoder_fwd / decoder_fwd), and rb_stream6, rb_stream128m and the persistent LSTM run as always.
      * Mimi: attention16_kernel and the row-mode tap_gemm8 linears (one launch over the merged [B*T, H] row matrix: B1, J1, s1)
        run as always.  The stem and head folds (rb_stream6m<stem> / <head>) do NOT run under the hook -- it wants the stem's output
        and the last block's output as tensors -- so the first and last 64-channel blocks are judged as rb_stream6m<> + the thin
        stem / head kernels; the folds keep tests/test_round6_kernels_gpu.py.
      * DAC: dac_unit6 (the 96-channel residual unit as one kernel) does NOT run under the hook (dac_path.hip dac_unit_fused returns
        false while it is armed): every residual unit is judged as its two tap-GEMM launches, the dilated k7 conv through the
        wide-slab `dil` instantiation.  dac_unit6 is checked to run without the hook; its arithmetic keeps the end-to-end DAC tests.
      * WavTokenizer: the backbone's linears are tap-GEMMs over the merged row matrix."""
    cfg, sd, W, W64 = _weights(name, request)
    codec = _codec(name, None, request)
    sig = _signal(name, "A").cuda()
    toks = codec.sig_to_toks(sig)
    names = _names_under_hook(codec, sig, toks, detail=name in ("mimi", "wavtokenizer"))
    base = {n.split("<")[0] for n in names}
    print(name, sorted(names))
    if name == "encodec":
        nat = next(iter(codec._natives.values()))
        assert nat.lib.ac_lstm_status(nat.h) == 1
        assert {"rb_stream6_kernel", "rb_stream128m_kernel", "enc_stream_kernel", "dec_stream_kernel", "lstm_persist16_kernel"} <= base, names
    elif name == "mimi":
        rows = sig.shape[0] * toks.shape[1] * 2
        assert "attention16_kernel" in base and "rb_stream128m_kernel" in base, names
        assert any(re.match(rf"tap_gemm8_kernel<.*> B1 M{rows} N\d+ K\d+ J1 s1$", n) for n in names), names
        assert "rb_stream6m_kernel<stem>" not in names and "rb_stream6m_kernel<head>" not in names, names
        plain = {s[0] for s in codec.profile_kernels(lambda: codec.toks_to_sig(codec.sig_to_toks(sig)))}
        assert {"rb_stream6m_kernel<stem>", "rb_stream6m_kernel<head>", "attention16_kernel"} <= plain, plain
    elif name == "dac":
        assert "dac_unit6_kernel" not in base and any(n.startswith("tap_gemm6_kernel") and ", dil>" in n for n in names), names
        plain = {s[0].split("<")[0] for s in codec.profile_kernels(lambda: codec.toks_to_sig(codec.sig_to_toks(sig)))}
        assert "dac_unit6_kernel" in plain, plain
    else:
        rows = sig.shape[0] * toks.shape[1]
        assert any(re.match(rf"tap_gemm\d_kernel<.*> B1 M{rows} N\d+ K\d+ J1 s1$", n) for n in names), names
