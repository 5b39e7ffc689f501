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

The layers that leave through the call's RESULT instead of the hook -- the last conv of EnCodec's / WavTokenizer's encoder
(`sig_to_feats`) and the head of every decoder (`toks_to_sig`: EnCodec's head inside dec_stream, head4_kernel for DAC and Mimi,
WavTokenizer's ISTFT head: Linear, polar_kernel, the inverse-rFFT GEMM, istft_env_kernel) -- are judged as the LAST layer of their
direction, in the same way and under the same bar: ref64 = result_fn(last tap.double()) against what the call returned
(layer_cases.result_tap_of).  For the two encoders the last tap and the result come from a second capture around `sig_to_feats`,
whose taps must equal those of the `sig_to_toks` capture bit for bit (the same encoder run twice).
`test_wavtok_istft_head_clipped_and_wrapped` puts the ISTFT head where the full-size checkpoint never takes it: magnitudes past
the clip at 100, phases past 2 pi, and clips so short that every output sample lies in the trimmed edge of the envelope.
DAC's 96-channel residual units run as dac_unit6_kernel under the hook (split16) and are judged as such;
`test_dac_residual_units_as_two_launches` holds the two tap-GEMM launches they replace to the same bar.
What the hook changes in the route, and what is still not judged alone (Mimi's stem and head folds), is listed in
`test_production_kernels_run_under_the_hook`."""
import math
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


def _judge(t, direction, case, got, ref64, ref32, figures, failures, named_rows=()):
    """One layer: the bar, the two figures, the printout; a failure message is appended to `failures`."""
    err = (got.double() - ref64).abs()
    amax = float(ref64.abs().max())
    tol = 5e-6 * max(1.0, amax) + 2e-5 * ref64.abs()
    e_gpu, e_ref = _rms(got.double() - ref64) / max(_rms(ref64), 1e-300), _rms(ref32.double() - ref64) / max(_rms(ref64), 1e-300)
    figures[t.name] = {"e_gpu": e_gpu, "e_ref": e_ref, "ratio": e_gpu / max(e_ref, 1e-300), "worst_err_over_tol": float((err / tol).max())}
    print(f"{case} {direction} {t.name:>28}: e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  ratio {e_gpu / max(e_ref, 1e-300):6.2f}  "
          f"worst |err|/tol {float((err / tol).max()):.3f}  max|ref64| {amax:.3e}" + ("  (result)" if t.result else ""))
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


def isolate(name, cfg, W, W64, direction, flat, x0, case, only=None, named_rows=(), result=None, record_as=None):
    """Walk the capture `flat` of one call: per layer, fp64 and fp32 references from the GPU's own previous tap, the bar, the two
    figures.  `only(tap)`: recompute just these layers (the others' sizes come from a dry run).  `result`: what the captured call
    returned ([B,N,D] features or [B,T] samples, on the CPU) -- checked as the last layer, from the last tap.  `record_as`: the parity
    record's codec key where it is not `name` (a second config of the same codec).  Returns the failure messages."""
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
        if check:
            _judge(t, direction, case, got, ref64, ref32, figures, failures, named_rows)
    assert off == flat.size, f"{case}: {flat.size - off} captured floats beyond the tap list"
    if result is not None:
        t = LC.result_tap_of(name, cfg, direction)
        assert t is not None and t.result and t.src == taps[-1].name, (name, direction)
        x = vals[t.src]
        with torch.no_grad():
            ref64 = f64[t.name](x.double())
            ref32 = f32[t.name](x)
        assert result.dtype == torch.float32 and tuple(result.shape) == tuple(ref64.shape), f"{case}: result {tuple(result.shape)}, the oracle's {tuple(ref64.shape)}"
        assert bool(torch.isfinite(result).all()), f"{case}: the {direction} result is not finite"
        _judge(t, direction, case, result, ref64, ref32, figures, failures)
    parity_record.record(record_as or name, f"layer_isolation/{case}/{direction}", per_layer=figures)
    return failures


def _captured_decode(codec, toks, fused_units=None):
    """toks_to_sig under the hook -> (waveform, capture).  `fused_units` (DAC): the very call that is judged must have run its
    96-channel residual units as dac_unit6_kernel (True) or as the two tap-GEMM launches (False) -- the two routes can agree to the
    bit (a power-of-two scale does not change an fp16 plane's rounding outside the subnormals), so the figures cannot tell."""
    out = []
    stats = codec.profile_kernels(lambda: out.append(capture(codec, lambda: codec.toks_to_sig(toks.cuda()), 1 << 26)))
    if fused_units is not None:
        names = {s[0] for s in stats}
        assert ({"dac_unit6_kernel<3>", "dac_unit6_kernel<3, dil>"} <= names) == fused_units, names
        assert any(n.startswith("dac_unit6_kernel") for n in names) == fused_units, names
    return out[0]


def _run_case(name, precision, which, request):
    cfg, sd, W, W64 = _weights(name, request)
    codec = _codec(name, precision, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    case = f"{name}/{precision or 'split16'}/{which}"
    sig = _signal(name, which)
    _, flat = capture(codec, lambda: codec.sig_to_toks(sig.cuda()), 1 << 26)
    feats = None
    if LC.result_tap_of(name, cfg, "encode") is not None:
        # the encoder's last conv leaves through sig_to_feats: the same encoder once more, so its taps are the first capture's to the bit
        feats, flat2 = capture(codec, lambda: codec.sig_to_feats(sig.cuda()), 1 << 26)
        assert flat2.shape == flat.shape and np.array_equal(flat2, flat), f"{case}: the taps of sig_to_feats differ from those of sig_to_toks"
        feats = feats.cpu()
    failures = isolate(name, cfg, W, W64, "encode", flat, sig[:, None], case, result=feats)
    toks = _oracle_tokens(name, which, request)
    x0 = _dequantised(name, codec, cfg, W, toks)
    rec, flat = _captured_decode(codec, toks, fused_units=(precision is None) if name == "dac" else None)
    assert bool(torch.isfinite(rec).all())
    failures += isolate(name, cfg, W, W64, "decode", flat, x0, case, result=rec.cpu())
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


@pytest.mark.parametrize("which", ["A", "B"])
def test_dac_residual_units_as_two_launches(which, request):
    """With `ac_debug_set "dac_unit" 0` DAC's 96-channel residual units (the last decoder block) run as the two tap-GEMM launches
    that dac_unit6_kernel replaces -- the route of every other unit width, and of these three under "fp32_exact".  The split16
    decode of the parametrised test above judges the fused kernel; this one holds the route it displaced to the same bar."""
    from audiocodecs_amd._native import debug_set

    cfg, sd, W, W64 = _weights("dac", request)
    codec = _codec("dac", None, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    toks = _oracle_tokens("dac", which, request)
    x0 = _dequantised("dac", codec, cfg, W, toks)
    debug_set(codec, "dac_unit", 0)
    try:
        rec, flat = _captured_decode(codec, toks, fused_units=False)
    finally:
        debug_set(codec, "dac_unit", 1)
    failures = isolate("dac", cfg, W, W64, "decode", flat, x0, f"dac/split16-two-launch/{which}", result=rec.cpu())
    assert not failures, "\n".join(failures)


HEAD_GAIN = 4.0          # on head.out: log-magnitudes and phases x 4 (x 16 would bring the fp32 oracle itself to 0.73 of the bar)
HEAD_TOKEN_SEED = 9305


@pytest.mark.parametrize("precision", PRECISIONS, ids=["split16", "fp32_exact"])
@pytest.mark.parametrize("N", [1, 2, 11])
def test_wavtok_istft_head_clipped_and_wrapped(N, precision, request):
    """WavTokenizer's ISTFT head (Linear -> polar_kernel -> inverse-rFFT GEMM -> istft_env_kernel) alone against fp64 where the
    synthetic checkpoint never takes it: there the largest log-magnitude is 2.8 against the clip at ln 100 = 4.6 and the largest
    |phase| 3.2 rad, so neither `min(exp(m), 100)` nor the range reduction of sincosf is ever exercised.  A second codec from the
    same state dict with head.out.weight / .bias x 4 decodes B = 2 random tokens (seed 9305); only the `sig` layer is judged, from
    the GPU's own `final` tap, under the per-tap bar.  Asserted on the fp64 reference's own intermediate values: at least 1 % of the
    bins are clipped (5.2 - 5.7 % on the CPU) and max|phase| > 2 pi (9.8 - 11.1).  The fp32 oracle's head sits at 0.07 - 0.23 of the
    bar on these inputs.  N = 1 and N = 2: n_fft = 4 hops, so every output sample lies in the trimmed "same" edge of the
    overlap-add envelope (fewer than four frames cover it); N = 11 has an interior."""
    import torch.nn.functional as F

    cfg, sd, _, _ = _weights("wavtokenizer", request)
    if ("head4", precision) not in _CACHE:
        from audiocodecs_amd import WavTokenizer

        sd4 = dict(sd)
        for k in ("head.out.weight", "head.out.bias"):
            sd4[k] = sd[k] * HEAD_GAIN
        O = _oracle("wavtokenizer")
        codec = WavTokenizer(24000, state_dict=sd4, arch=cfg, precision=precision).eval()
        codec.sig_to_toks(noise(1, 1, 4800).cuda())          # creates the native handle
        _CACHE["head4", precision] = (codec, O.cast_weights(sd4), O.cast_weights(sd4, torch.float64))
    codec, W, W64 = _CACHE["head4", precision]
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    B, C = 2, cfg.backbone_dim
    toks = torch.randint(0, cfg.codebook_size, (B, N, 1), generator=torch.Generator().manual_seed(HEAD_TOKEN_SEED))
    rec, flat = capture(codec, lambda: codec.toks_to_sig(toks.cuda()), 1 << 22)
    rec = rec.cpu()
    taps = LC.taps_of("wavtokenizer", cfg, "decode")
    res = LC.result_tap_of("wavtokenizer", cfg, "decode")
    assert res.oracle == "sig" and res.src == taps[-1].name == "final"
    assert flat.size == len(taps) * B * N * C, (flat.size, len(taps), B, N, C)       # every backbone tap is [B][N][backbone_dim]
    final = torch.from_numpy(flat[-B * N * C :]).view(B, N, C).transpose(1, 2)      # the oracle's [B,C,N]
    with torch.no_grad():
        ref64 = LC.layer_fns("wavtokenizer", cfg, W64, "decode")["sig"](final.double())
        ref32 = LC.layer_fns("wavtokenizer", cfg, W, "decode")["sig"](final)
        logmag, phase = F.linear(final.double().transpose(1, 2), W64["head.out.weight"], W64["head.out.bias"]).chunk(2, dim=-1)
    clipped, wrap = float((logmag > math.log(100.0)).double().mean()), float(phase.abs().max())
    print(f"N {N}: {100 * clipped:.1f} % of the bins clipped, max|phase| {wrap:.2f} rad, max log-magnitude {float(logmag.max()):.2f}")
    assert clipped >= 0.01 and wrap > 2 * math.pi, (clipped, wrap)
    assert tuple(rec.shape) == tuple(ref64.shape) == (B, N * cfg.hop_length) and bool(torch.isfinite(rec).all())
    failures, figures = [], {}
    case = f"wavtokenizer/{precision or 'split16'}/head_x4_N{N}"
    _judge(res, "decode", case, rec, ref64, ref32, figures, failures)
    parity_record.record("wavtokenizer", f"layer_isolation/{case}/decode", per_layer=figures)
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
        Result layers: the encoder's last conv is a tap-GEMM of K = 7 x 512 over the frames; the head is inside dec_stream.
      * Mimi: attention16_kernel and the row-mode tap_gemm8 linears (one launch over the merged [B*T, H] row matrix: B1, J1, s1)
        run as always.  The stem and head folds (rb_stream6m<stem> / <head>) do NOT run under the hook -- it wants the stem's output
        and the last block's output as tensors, and the folds' inputs are not observable in the un-hooked route -- so the first and
        last 64-channel blocks are judged as rb_stream6m<> + the thin stem / head kernels.  STILL NOT JUDGED ALONE against fp64:
        those two folds; they stay kernel-against-kernel in tests/test_round6_kernels_gpu.py.  What they are compared with there --
        head4_kernel after rb_stream6m<> -- is what the result layer `decoder.layers.14` pins to fp64 here.
      * DAC: the three 96-channel residual units of the last decoder block run as dac_unit6_kernel under the hook as without it
        (dilations 1, 3, 9: the <3> and <3, dil> instantiations) and are judged as that kernel; with `ac_debug_set "dac_unit" 0`
        they are the two tap-GEMM launches, the dilated k7 conv through the wide-slab `dil` instantiation
        (test_dac_residual_units_as_two_launches).  Both routes are pinned here.  Result layer: head4_kernel.
      * WavTokenizer: the backbone's linears are tap-GEMMs over the merged row matrix.  Result layers: the encoder's last conv
        as EnCodec's; the ISTFT head's polar_kernel and istft_env_kernel around its two tap-GEMMs."""
    cfg, sd, W, W64 = _weights(name, request)
    codec = _codec(name, None, request)
    sig = _signal(name, "A").cuda()
    toks = codec.sig_to_toks(sig)
    names = _names_under_hook(codec, sig, toks, detail=True)
    base = {n.split("<")[0] for n in names}
    print(name, sorted(names))
    D = {"encodec": 128, "wavtokenizer": 512}.get(name)
    last_conv = rf"tap_gemm\w*_kernel<.*> B\d+ M\d+ N{D} K{7 * 512} "      # the encoders' ELU -> Conv1d(512, D, k7)
    if name == "encodec":
        nat = next(iter(codec._natives.values()))
        assert nat.lib.ac_lstm_status(nat.h) == 1
        assert {"rb_stream6_kernel", "rb_stream128m_kernel", "enc_stream_kernel", "dec_stream_kernel", "lstm_persist16_kernel"} <= base, names
        assert any(re.match(last_conv, n) for n in names), names
    elif name == "mimi":
        rows = sig.shape[0] * toks.shape[1] * 2
        assert "attention16_kernel" in base and "rb_stream128m_kernel" in base, names
        assert any(re.match(rf"tap_gemm8_kernel<.*> B1 M{rows} N\d+ K\d+ J1 s1$", n) for n in names), names
        assert "rb_stream6m_kernel<stem>" not in names and "rb_stream6m_kernel<head>" not in names, names
        assert "head4_kernel" in base, names
        plain = {s[0] for s in codec.profile_kernels(lambda: codec.toks_to_sig(codec.sig_to_toks(sig)))}
        assert {"rb_stream6m_kernel<stem>", "rb_stream6m_kernel<head>", "attention16_kernel"} <= plain, plain
    elif name == "dac":
        from audiocodecs_amd._native import debug_set

        assert {"dac_unit6_kernel<3>", "dac_unit6_kernel<3, dil>"} <= names and "head4_kernel" in base, names
        assert any(n.startswith("tap_gemm6_kernel") and ", dil>" in n for n in names), names      # the wider units' dilated convs
        plain = {s[0] for s in codec.profile_kernels(lambda: codec.toks_to_sig(codec.sig_to_toks(sig)))}
        assert {"dac_unit6_kernel<3>", "dac_unit6_kernel<3, dil>"} <= plain, plain
        debug_set(codec, "dac_unit", 0)
        try:
            two = _names_under_hook(codec, sig, toks)
        finally:
            debug_set(codec, "dac_unit", 1)
        assert not any(n.startswith("dac_unit6_kernel") for n in two), two
        assert any(n.startswith("tap_gemm6_kernel") and ", dil>" in n for n in two) and "head4_kernel" in two, two
    else:
        rows = sig.shape[0] * toks.shape[1]
        assert any(re.match(rf"tap_gemm\d_kernel<.*> B1 M{rows} N\d+ K\d+ J1 s1$", n) for n in names), names
        assert any(re.match(last_conv, n) for n in names), names
        assert {"polar_kernel", "istft_env_kernel"} <= base, names
