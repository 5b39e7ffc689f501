"""rb256_fused_kernel (csrc/rb256_fused.h): EnCodec's 256-channel residual block as one kernel that reads the producer's raw rows,
against the two tap-GEMM launches it replaces (ac_debug_set "rb256_fused" = 0) and against fp64.

The block alone is reached through the capture hook of a full-config encode: tap enc9 is the block's input exactly as the kernel saw
it (the x5 down conv's raw output), tap enc10 its raw output; one row of that stage is 40 samples, so T = 40 * rows puts `rows` rows
per clip in front of the block.  The kernel's tile is 128 rows; below one tile the two-launch path runs under either setting (core.hip
rb256_ok), so the short cases hold the routing and the reflect rule's small-input case of that path.

The two paths do NOT agree bit for bit: stage A's accumulators do (same operand planes, same k order), but the hidden activation is
split with the scale of the derived bound |hidden| <= hb0 + hb1 amax(x) where the two-launch path uses the hidden tensor's measured
amax.  So each path is held to fp64 on its own, with the per-tap bar of tests/test_layer_isolation_gpu.py WITHOUT its relative term,

    |got - ref64| <= 5e-6 * max(1, max|ref64|)        elementwise,

and the whole codec to equal tokens and <= 1e-5 RMS between the waveforms of the two paths."""
import numpy as np
import pytest
import torch

import layer_cases as LC
from golden_cases import noise
from test_gpu_parity import capture

pytestmark = pytest.mark.gpu

TILE = 128
ROWS = [1, 2, 3, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]
SAMPLES_PER_ROW = 40          # 2 * 4 * 5: the strides in front of the encoder's 256-channel stage
_CACHE = {}


def _setup(request):
    if "codec" not in _CACHE:
        from audiocodecs_amd import Encodec
        from oracle import encodec_oracle as O

        cfg, sd = request.getfixturevalue("checkpoints")("full", 0)
        codec = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
        codec.sig_to_toks(noise(1, 1, 4800).cuda())          # creates the native handle
        W64 = O.fold_weight_norm(sd, torch.float64)
        _CACHE["codec"] = (cfg, codec, LC.layer_fns("encodec", cfg, W64, "encode")["enc10"])
    return _CACHE["codec"]


def _switch(codec, value):
    from audiocodecs_amd._native import debug_set

    debug_set(codec, "rb256_fused", value)


def _block_taps(cfg, codec, sig, length=None):
    """-> (enc9, enc10, kernel names) of one encode, the taps as [B,C,L] tensors."""
    taps = LC.taps_of("encodec", cfg, "encode")
    assert [t.name for t in taps] == ["enc0", "enc1", "enc3", "enc4", "enc6", "enc7", "enc9", "enc10", "enc12", "enc13"]
    B, T = sig.shape
    shape, rows, c = {"enc0": (B, 32, T)}, T, 32
    for i, ratio in zip((1, 4, 7, 10), (2, 4, 5, 8)):     # residual block enc<i>, then the down conv enc<i + 2>
        shape[f"enc{i}"] = (B, c, rows)
        rows, c = -(-rows // ratio), 2 * c
        shape[f"enc{i + 2}"] = (B, c, rows)
    shape["enc13"] = (B, c, rows)
    out = []
    stats = codec.profile_kernels(lambda: out.append(capture(codec, lambda: codec.sig_to_toks(sig.cuda(), None if length is None else length.cuda()), 1 << 24)))
    got = LC.split_capture(out[0][1], taps, lambda t: shape[t.name])
    return torch.from_numpy(np.ascontiguousarray(got["enc9"])), torch.from_numpy(np.ascontiguousarray(got["enc10"])), {s[0] for s in stats}


def _both_paths(request, sig, length=None):
    cfg, codec, f64 = _setup(request)
    try:
        _switch(codec, 1)
        x_on, y_on, names_on = _block_taps(cfg, codec, sig, length)
        _, y_again, _ = _block_taps(cfg, codec, sig, length)
        _switch(codec, 0)
        x_off, y_off, names_off = _block_taps(cfg, codec, sig, length)
    finally:
        _switch(codec, 1)
    assert ("rb256_fused_kernel" in names_on) == (x_on.shape[2] >= TILE) and "rb256_fused_kernel" not in names_off, (sorted(names_on), sorted(names_off))
    assert torch.equal(x_on, x_off), "the producer's raw rows depend on how many flavours it writes"
    assert torch.equal(y_on, y_again), "two runs of the block on the same rows differ"
    with torch.no_grad():
        ref = f64(x_on.double())
    bar = 5e-6 * max(1.0, float(ref.abs().max()))
    e_on, e_off = float((y_on.double() - ref).abs().max()), float((y_off.double() - ref).abs().max())
    print(f"rows {x_on.shape[2]}: max|on - ref64| {e_on:.3e}  max|off - ref64| {e_off:.3e}  bar {bar:.3e}  max|on - off| {float((y_on - y_off).abs().max()):.3e}  "
          f"bit-equal {bool(torch.equal(y_on, y_off))}")
    assert bool(torch.isfinite(y_on).all()) and e_on <= bar, (e_on, bar)
    assert e_off <= bar, (e_off, bar)
    return y_on, y_off


@pytest.mark.parametrize("rows", ROWS)
def test_block_alone_against_two_launches_and_fp64(rows, request):
    sig = noise(4100 + rows, 2, SAMPLES_PER_ROW * rows)
    y_on, y_off = _both_paths(request, sig)
    assert y_on.shape == (2, 256, rows)
    if rows < TILE:       # below one tile the switch changes nothing
        assert torch.equal(y_on, y_off)


def test_block_in_a_ragged_batch(request):
    sig = noise(4201, 2, SAMPLES_PER_ROW * (2 * TILE + 5))
    _both_paths(request, sig, torch.tensor([1.0, 0.6]))


def test_whole_codec_with_the_kernel_and_without(request):
    from audiocodecs_amd._native import debug_set

    cfg, codec, _ = _setup(request)
    B, T = 2, TILE * 160 + 321
    sig = noise(4301, B, T).cuda()
    run = lambda: codec.toks_to_sig(codec.sig_to_toks(sig))
    try:
        debug_set(codec, "prof_detail", 1)
        _switch(codec, 1)
        toks_on = codec.sig_to_toks(sig)
        rec_on = codec.toks_to_sig(toks_on)
        assert torch.equal(toks_on, codec.sig_to_toks(sig)) and torch.equal(rec_on, codec.toks_to_sig(toks_on))       # re-runs
        stats_on = codec.profile_kernels(run)
        _switch(codec, 0)
        toks_off = codec.sig_to_toks(sig)
        rec_off = codec.toks_to_sig(toks_off)
        stats_off = codec.profile_kernels(run)
    finally:
        _switch(codec, 1)
        debug_set(codec, "prof_detail", 0)
    assert torch.equal(toks_on, toks_off)
    d = float((rec_on.double() - rec_off.double()).pow(2).mean().sqrt())
    print(f"waveform rms(on - off) {d:.3e}  bit-equal {bool(torch.equal(rec_on, rec_off))}")
    assert d <= 1e-5
    # the kernel is what ran: once in the encoder, once in the decoder, in place of the four tap-GEMM launches
    on = {s[0]: s for s in stats_on}
    off = {s[0]: s for s in stats_off}
    assert on["rb256_fused_kernel"][1] == 2 and "rb256_fused_kernel" not in off, (sorted(on), sorted(off))
    M_enc, N_dec = -(-T // SAMPLES_PER_ROW), -(-T // 320)
    block = [f" B{B} M{M_enc} N128 K768 J3", f" B{B} M{M_enc} N256 K384 J1", f" B{B} M{8 * N_dec} N128 K768 J3", f" B{B} M{8 * N_dec} N256 K384 J1"]
    for shape in block:
        assert not any(shape in n for n in on), (shape, sorted(on))
        assert sum(off[n][1] for n in off if shape in n) == 1, (shape, sorted(off))
    # the x5 down conv and the x8 up conv wrote ONE flavour: bytes of a record = inputs + outputs x flavours + weights (core.hip run_tap)
    for shape, inb, M, N, K in ((f" B{B} M{M_enc} N256 K1280 J2 s5", B * -(-T // 8) * 128 * 4, M_enc, 256, 1280),
                                (f" B{B} M{N_dec} N2048 K1024 J2 s1", B * N_dec * 512 * 4, N_dec, 2048, 1024)):
        r_on = [on[n] for n in on if shape in n]
        r_off = [off[n] for n in off if shape in n]
        assert len(r_on) == 1 and len(r_off) == 1 and r_on[0][1] == 1 and r_off[0][1] == 1, (shape, sorted(on))
        out = B * M * N * 4
        assert r_on[0][4] == inb + out + N * K * 4, (shape, r_on[0][4], inb, out)
        assert r_off[0][4] == inb + 2 * out + N * K * 4, (shape, r_off[0][4], inb, out)
