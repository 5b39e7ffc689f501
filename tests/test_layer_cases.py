"""CPU checks of tests/layer_cases.py and of the oracles' layer lists (oracle/*_oracle.py `encoder_layers`, `decoder_layers`,
Mimi's `transformer_layers` / `downsample` / `upsample`) on the tiny fixtures:

  * the tap lists name tensors the fixtures hold, in an order whose shapes agree with the fixtures' `act_shapes` and whose sizes
    sum to what the capture hook emits for that call (the sum the GPU tap tests walk);
  * running the lists ONE LAYER AT A TIME -- each layer on the previous layer's output, as the monolithic encoder / decoder used
    to -- reproduces the committed activations bit for bit in fp32.  Mimi's fixtures come from the reference's own modules, whose
    attention is another kernel than the oracle's restatement: from the first transformer layer on they agree to the 5e-6 of
    tests/test_mimi_oracle_golden.py, not to the bit (they did not before the layers became addressable either); everything
    upstream of it, and every tap of the other three codecs, is bit-equal;
  * the six result layers (`result_tap_of`: the layers that leave through the call's return value, not through the hook) close
    the lists: the tap functions folded from the input and then the result function give the oracle's own `sig_to_feats` /
    `toks_to_sig`, to the bit, in the layout of the return value."""
import numpy as np
import pytest
import torch

import dac_cases
import golden_cases
import layer_cases as LC
import mimi_cases
import wavtok_cases
from conftest import GOLDEN_DIR


def _setup(codec, name, request):
    """-> (cfg, W fp32, z, meta, encode INPUT [B,1,T], decode INPUT [B,hidden,N])"""
    if codec == "encodec":
        from oracle import encodec_oracle as O

        z, meta = request.getfixturevalue("golden")
        cfg, sd = request.getfixturevalue("checkpoints")("tiny", 0)
        W = O.fold_weight_norm(sd)
        inp = golden_cases.make_input(next(c for c in golden_cases.CASES if c["name"] == name), GOLDEN_DIR)
        sig = inp["sig"]
        x = (O.padding_mask(sig, inp.get("length", torch.ones(len(sig)))) * sig)[:, None]      # the hooks saw the masked pass
        codes = torch.from_numpy(z[f"{name}.toks"].astype(np.int64)).movedim(-1, 0)
        return cfg, W, z, meta, x, O.rvq_decode(O.codebooks(W, codes.shape[0]), codes)
    toks = None
    if codec == "mimi":
        from oracle import mimi_oracle as O

        z, meta = request.getfixturevalue("mimi_golden")
        cfg, sd = request.getfixturevalue("mimi_checkpoints")("tiny", 0)
        W = O.cast_weights(sd)
        sig = mimi_cases.make_input(next(c for c in mimi_cases.CASES if c["name"] == name), GOLDEN_DIR)["sig"]
        toks = torch.from_numpy(z[f"{name}.toks"].astype(np.int64))
        return cfg, W, z, meta, sig[:, None], O.rvq_decode(cfg, W, toks.movedim(-1, -2))
    if codec == "dac":
        from oracle import dac_oracle as O

        z, meta = request.getfixturevalue("dac_golden")
        cfg, sd = request.getfixturevalue("dac_checkpoints")("tiny", 0)
        W = O.cast_weights(sd)
        sig = dac_cases.make_input(next(c for c in dac_cases.CASES if c["name"] == name), GOLDEN_DIR)["sig"]
        toks = torch.from_numpy(z[f"{name}.toks"].astype(np.int64))
        return cfg, W, z, meta, sig[:, None], O.from_codes(cfg, W, toks.movedim(-1, -2))[0]
    from oracle import wavtokenizer_oracle as O

    z, meta = request.getfixturevalue("wavtok_golden")
    cfg, sd = request.getfixturevalue("wavtok_checkpoints")("tiny", 0)
    W = O.cast_weights(sd)
    sig = wavtok_cases.make_input(next(c for c in wavtok_cases.CASES if c["name"] == name), GOLDEN_DIR)["sig"]
    toks = torch.from_numpy(z[f"{name}.toks"].astype(np.int64))
    return cfg, W, z, meta, sig[:, None], O.toks_to_qfeats(cfg, W, toks).movedim(-1, -2)


def _fixture_values(z, meta, name, tap, v):
    """The fixture's array for `tap` and `v` (the oracle's tensor) brought to the same form: whole, or every act_stride-th element."""
    g = z[f"{name}.act.{tap.name}"]
    v = v.numpy()
    if g.shape != v.shape:           # stored flat: whole up to act_full_max elements, every act_stride-th beyond
        v = v.reshape(-1)
        v = v[:: (1 if v.size <= meta.get("act_full_max", 0) else meta["act_stride"])]
    return g, v


CASES = [("encodec", "tiny_taps"), ("encodec", "tiny_ragged"), ("mimi", "tiny_taps"), ("mimi", "tiny_odd"),
         ("dac", "tiny_taps"), ("dac", "tiny_odd"), ("wavtokenizer", "tiny_taps"), ("wavtokenizer", "tiny_odd")]


@pytest.mark.parametrize("codec,name", CASES, ids=[f"{c}-{n}" for c, n in CASES])
def test_layer_lists_reproduce_the_tiny_fixtures(codec, name, request):
    cfg, W, z, meta, x_enc, x_dec = _setup(codec, name, request)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    shapes = meta["cases"][name].get("act_shapes") if "cases" in meta and name in meta["cases"] else None
    for direction, x in (("encode", x_enc), ("decode", x_dec)):
        taps = LC.taps_of(codec, cfg, direction)
        fns = LC.layer_fns(codec, cfg, W, direction)
        res = LC.result_tap_of(codec, cfg, direction)
        assert [t.name for t in taps if not t.skip] + ([res.name] if res else []) == list(fns)
        assert not any(t.result for t in taps)           # taps_of is what the capture emits: no result layer in it
        vals, size, exact = {LC.INPUT: x}, 0, True
        for t in taps:
            if t.skip:                                   # the quantiser's output: the decoder's input, captured but no layer
                assert t.src == LC.INPUT and t.oracle is None
                vals[t.name] = vals[LC.INPUT]
                size += x.numel()
                continue
            assert f"{name}.act.{t.name}" in z.files, t.name
            with torch.no_grad():
                v = vals[t.name] = fns[t.name](vals[t.src])
            assert v.dtype == torch.float32
            size += v.numel()
            if shapes is not None:
                assert list(v.shape) == shapes[t.name], (t.name, list(v.shape), shapes[t.name])
            g, got = _fixture_values(z, meta, name, t, v)
            assert g.shape == got.shape, (t.name, g.shape, got.shape)
            if codec == "mimi" and t.layout == "BTH":
                exact = False                            # the reference's attention kernel is not the oracle's (module docstring)
            if exact:
                assert np.array_equal(got, g), (t.name, float(np.abs(got - g).max()))
            else:
                np.testing.assert_allclose(got, g, rtol=0, atol=5e-6, err_msg=t.name)
        # what the capture hook emits for this call, as the GPU tap tests count it: the fixtures' own shapes, one tensor per tap
        # (EnCodec's fixtures hold the whole tensors and WavTokenizer's every act_stride-th element, without a shape table: there the
        # per-tap shape comparison above is the check)
        if shapes is not None:
            assert size == sum(int(np.prod(shapes[t.name])) if not t.skip else int(x.numel()) for t in taps)
        # split_capture walks exactly these sizes and gives each tap back in its oracle layout
        flat = np.concatenate([(vals[t.name] if t.layout == "BTH" else vals[t.name].transpose(1, 2)).contiguous().numpy().reshape(-1) for t in taps])
        back = LC.split_capture(flat, taps, lambda t: vals[t.name].shape)
        for t in taps:
            assert np.array_equal(back[t.name], vals[t.name].numpy()), t.name
        with pytest.raises(AssertionError):
            LC.split_capture(flat[:-1], taps, lambda t: vals[t.name].shape)


RESULTS = [("encodec", "encode", "enc15", "enc13"), ("encodec", "decode", "dec15", "dec13"), ("wavtokenizer", "encode", "enc15", "enc13"),
           ("wavtokenizer", "decode", "sig", "final"), ("dac", "decode", "decoder.conv2", None), ("mimi", "decode", "decoder.layers.14", None)]


@pytest.mark.parametrize("name", ["tiny_taps", "tiny_odd"])
@pytest.mark.parametrize("codec,direction,full_oracle,full_src", RESULTS, ids=[f"{c}-{d}" for c, d, _, _ in RESULTS])
def test_result_layers_close_the_lists(codec, direction, full_oracle, full_src, name, request):
    """Taps folded from the input, then the result layer == the oracle's own entry point, bit for bit; and the names at the
    full-size configs are the ones the oracles' lists end with."""
    import importlib

    name = "tiny_ragged" if codec == "encodec" and name == "tiny_odd" else name
    cfg, W, z, meta, x_enc, x_dec = _setup(codec, name, request)
    torch.set_num_threads(min(8, torch.get_num_threads()))
    O = importlib.import_module({"encodec": "oracle.encodec_oracle", "mimi": "oracle.mimi_oracle", "dac": "oracle.dac_oracle",
                                 "wavtokenizer": "oracle.wavtokenizer_oracle"}[codec])
    taps, fns = LC.taps_of(codec, cfg, direction), LC.layer_fns(codec, cfg, W, direction)
    res = LC.result_tap_of(codec, cfg, direction)
    assert res is not None and res.result and not res.skip and res.src == taps[-1].name and list(fns)[-1] == res.name
    vals = {LC.INPUT: x_enc if direction == "encode" else x_dec}
    with torch.no_grad():
        for t in taps:
            vals[t.name] = vals[LC.INPUT] if t.skip else fns[t.name](vals[t.src])
        got = fns[res.name](vals[res.src])
        if direction == "encode":
            want = O.sig_to_feats(cfg, W, x_enc[:, 0])
            assert res.layout == "BND" and want.shape == (x_enc.shape[0], vals[res.src].shape[2], want.shape[2])
        else:
            want = O.toks_to_sig(cfg, W, torch.from_numpy(z[f"{name}.toks"].astype(np.int64)))
            assert res.layout == "BT" and want.dim() == 2
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want), float((got - want).abs().max())
    # the full-size configs: the names the oracles' lists end with
    fx = {"encodec": "checkpoints", "mimi": "mimi_checkpoints", "dac": "dac_checkpoints", "wavtokenizer": "wavtok_checkpoints"}[codec]
    full = request.getfixturevalue(fx)("full", 0)[0]
    rf = LC.result_tap_of(codec, full, direction)
    assert rf.oracle == full_oracle and rf.src == LC.taps_of(codec, full, direction)[-1].name
    if full_src:
        assert rf.src == full_src
    if codec in ("dac", "mimi"):      # their encoders end in a captured tap
        assert LC.result_tap_of(codec, cfg, "encode") is None and LC.result_tap_of(codec, full, "encode") is None


def test_mimi_transformer_layer_offset_and_names(mimi_checkpoints):
    """A transformer layer fn takes the position of its first row: rows [k:] of a pass from 0 equal a pass over x[k:] started
    at pos0 = k wherever the window hides the cut (k >= sliding_window rows later every key is inside the chunk)."""
    from oracle import mimi_oracle as O

    cfg, sd = mimi_checkpoints("tiny", 0)
    W = O.cast_weights(sd, torch.float64)
    win = cfg.sliding_window
    x = torch.randn(1, 3 * win, cfg.hidden_size, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    name, fn = O.transformer_layers(cfg, W, "encoder_transformer")[0]
    assert name == "encoder_transformer.layers.0"
    full = fn(x)
    assert torch.equal(full, fn(x, 0))
    k = win + 1
    part = fn(x[:, k:], k)
    assert torch.allclose(part[:, win - 1 :], full[:, k + win - 1 :], atol=1e-12)
    # (RoPE scores depend on position differences only, so the layer's OUTPUT cannot show pos0; the tables do)
    c0, s0 = O.rope_tables(cfg, 7, torch.float64)
    c3, s3 = O.rope_tables(cfg, 4, torch.float64, 3)
    assert torch.equal(c0[3:], c3) and torch.equal(s0[3:], s3) and not torch.equal(s0[:4], s3)


def test_range_input_has_the_gains_of_the_split16_cases():
    sig = golden_cases.noise(1, 3, 12000)
    burst = golden_cases.noise(2, 1, 400)[0]
    assert LC.gain_input(sig, "A", burst) is sig
    b = LC.gain_input(sig, "B", burst)
    assert torch.equal(b[0], sig[0] * 1e-3) and torch.equal(b[2], sig[2] * 50.0)
    quiet = sig[1] * 1e-3
    assert torch.equal(b[1, :4000], quiet[:4000]) and torch.equal(b[1, 4400:], quiet[4400:])
    assert float(b[1, 4000:4400].abs().max()) > 1000 * float(quiet.abs().max())
    b2 = LC.gain_input(sig[:2], "B", burst)
    assert torch.equal(b2[1], sig[1] * 50.0) and float(b2[0].abs().max()) > 1.0
