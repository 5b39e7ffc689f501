"""CPU tests of the DNSMOS feature (audiocodecs_amd.dnsmos): the window plan against a literal restatement of the reference's loop, the
protobuf wire reader on a blob assembled here, the fp64 statement (tests/dnsmos_ref.py) against its pins -- torch.stft, transformers'
Slaney filterbank, the values in tests/golden/dnsmos_golden.npz -- and every refusal that needs no GPU."""
import os

import numpy as np
import pytest
import torch

import dnsmos_ref as R

PLAN_LENGTHS = [1, 159, 72080, 144159, 144160, 159999, 160000, 271999, 272000, 400000, 527999, 528000, 655360]


# ---- plan -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L16", PLAN_LENGTHS)
def test_plan_is_the_reference_loop(L16):
    from audiocodecs_amd.dnsmos import WINDOW, dnsmos_segments

    starts = dnsmos_segments(L16)
    wins = R.reference_windows(np.arange(L16, dtype=np.int64))       # sample j carries its own index: a window shows start and modulus
    assert len(starts) == len(wins) >= 1 and starts[0] == 0
    j = np.arange(WINDOW, dtype=np.int64)
    for s, w in zip(starts, wins):
        assert len(w) == WINDOW == 144160
        assert np.array_equal(w, (s + j) % L16)


def test_plan_skips_the_windows_the_float_arithmetic_shortens():
    from audiocodecs_amd.dnsmos import dnsmos_segments

    first7 = tuple(16000 * i for i in range(7))
    assert dnsmos_segments(4000) == first7                           # doubled six times to 256000 samples: 7 hops, all whole
    assert dnsmos_segments(144159) == first7                         # doubled once: 288318 samples, 9 hops, windows 7 and 8 are 144159 long
    assert dnsmos_segments(144160) == (0,)
    assert dnsmos_segments(271999) == first7
    assert dnsmos_segments(272000) == first7                         # 8 hops; window 7 is int(16.01 * 16000) - 112000 = 144159 long: skipped
    assert dnsmos_segments(528000) == first7                         # 24 hops: windows 7 .. 23 all skipped
    assert dnsmos_segments(544000) == first7 + (16000 * 24,)         # the first kept window after the gap
    assert dnsmos_segments(655360) == first7 + tuple(16000 * i for i in range(24, 31))
    with pytest.raises(ValueError):
        dnsmos_segments(0)


# ---- reader -----------------------------------------------------------------------------------------------------------------------------
def _vi(v):
    out = b""
    while True:
        b = v & 0x7F
        v >>= 7
        out += bytes([b | (0x80 if v else 0)])
        if not v:
            return out


def _ld(field, payload):
    return _vi(field << 3 | 2) + _vi(len(payload)) + payload


def _attr_ints(name, ints):
    return _ld(5, _ld(1, name.encode()) + b"".join(_vi(8 << 3) + _vi(i) for i in ints) + _vi(20 << 3) + _vi(7))


def _attr_int(name, i):
    return _ld(5, _ld(1, name.encode()) + _vi(3 << 3) + _vi(i) + _vi(20 << 3) + _vi(2))


def _node(op, ins, outs, attrs=b""):
    return _ld(1, b"".join(_ld(1, s.encode()) for s in ins) + b"".join(_ld(2, s.encode()) for s in outs) + _ld(4, op.encode()) + attrs)


def _init(name, arr, raw):
    body = b"".join(_vi(1 << 3) + _vi(d) for d in arr.shape) + _vi(2 << 3) + _vi(1)
    data = arr.astype("<f4").tobytes()
    body += _ld(9, data) if raw else _ld(4, data)                    # raw_data, or float_data packed
    return _ld(5, body + _ld(8, name.encode()))


def _model(weights, drop=None, pool_kernel=(2, 2)):
    """An ONNX blob of the P.808 chain with `weights`, assembled field by field (conv tensors as float_data, dense as raw_data)."""
    conv = _attr_ints("dilations", [1, 1]) + _attr_int("group", 1) + _attr_ints("kernel_shape", [3, 3]) + _attr_ints("pads", [1, 1, 1, 1]) + _attr_ints("strides", [1, 1])
    pool = _attr_ints("kernel_shape", list(pool_kernel)) + _attr_ints("strides", [2, 2])
    nodes, inits, cur = [], [], "input_1"

    def add(op, extra=(), attrs=b""):
        nonlocal cur
        nxt = f"t{len(nodes)}"
        nodes.append((op, _node(op, [cur, *extra], [nxt], attrs)))
        cur = nxt

    add("Unsqueeze", attrs=_attr_ints("axes", [3]))
    add("Transpose", attrs=_attr_ints("perm", [0, 3, 1, 2]))
    for name, pooled in (("conv5", True), ("conv6", True), ("conv7", False), ("conv8", True), ("conv9", False)):
        inits += [_init(name + "/kernel", weights[name + ".w"], False), _init(name + "/bias", weights[name + ".b"], False)]
        add("Conv", (name + "/kernel", name + "/bias"), conv)
        add("Relu")
        if pooled:
            add("MaxPool", attrs=pool)
    add("Transpose", attrs=_attr_ints("perm", [0, 2, 3, 1]))
    add("ReduceMax", attrs=_attr_ints("axes", [1, 2]) + _attr_int("keepdims", 0))
    for k, name in enumerate(("dense3", "dense4", "dense5")):
        inits += [_init(name + "/w", weights[name + ".w"], True), _init(name + "/b", weights[name + ".b"], True)]
        add("MatMul", (name + "/w",))
        add("Add", (name + "/b",))
        if k < 2:
            add("Relu")
    if drop is not None:
        del nodes[drop]
    graph = b"".join(n for _, n in nodes) + _ld(2, b"g") + b"".join(inits)
    return _vi(1 << 3) + _vi(7) + _ld(7, graph)


@pytest.fixture(scope="module")
def small_weights():
    from audiocodecs_amd.dnsmos import WEIGHT_SHAPES

    rng = np.random.default_rng(5)
    return {k: rng.standard_normal(s).astype(np.float32) for k, s in WEIGHT_SHAPES.items()}


def test_reader_reads_a_blob_assembled_here(small_weights):
    from audiocodecs_amd.dnsmos import CHAIN, read_onnx, weights_from_onnx

    blob = _model(small_weights)
    nodes, tensors = read_onnx(blob)
    assert [n["op"] for n in nodes] == [c[0] for c in CHAIN] and len(tensors) == 16
    assert nodes[2]["attrs"]["pads"] == [1, 1, 1, 1] and nodes[2]["attrs"]["group"] == 1 and nodes[16]["attrs"]["keepdims"] == 0
    got = weights_from_onnx(blob)
    assert set(got) == set(small_weights)
    for k, v in small_weights.items():
        assert got[k].dtype == np.float32 and np.array_equal(got[k], v), k


def test_reader_refuses_another_graph(small_weights):
    from audiocodecs_amd.dnsmos import weights_from_onnx

    with pytest.raises(ValueError, match="not the P.808 chain"):
        weights_from_onnx(_model(small_weights, drop=4))             # the first MaxPool is gone
    with pytest.raises(ValueError, match="kernel_shape"):
        weights_from_onnx(_model(small_weights, pool_kernel=(3, 3)))
    bad = dict(small_weights)
    bad["conv9.w"] = bad["conv9.w"][:32]
    with pytest.raises(ValueError, match="conv9.w"):
        weights_from_onnx(_model(bad))
    with pytest.raises(ValueError):
        weights_from_onnx(b"\x08\x07")                               # a model without a graph
    with pytest.raises(ValueError):
        weights_from_onnx(_model(small_weights)[:-7])                # truncated


def test_load_weights_reads_the_fixture_and_an_onnx(tmp_path, small_weights):
    from audiocodecs_amd.dnsmos import WEIGHT_SHAPES, DnsmosWeights, load_weights

    w = load_weights(os.path.join(R.GOLDEN, "dnsmos_p808.npz"))
    assert isinstance(w, DnsmosWeights) and {k: tuple(v.shape) for k, v in w.tensors.items()} == WEIGHT_SHAPES
    assert w.flat().numel() == 54945 and w.flat().dtype == torch.float32
    p = tmp_path / "m.onnx"
    p.write_bytes(_model(small_weights))
    w2 = load_weights(str(p))
    assert all(np.array_equal(w2.tensors[k].numpy(), small_weights[k]) for k in WEIGHT_SHAPES)
    with pytest.raises(ValueError):
        DnsmosWeights({k: v for k, v in small_weights.items() if k != "dense5.b"})


# ---- statement ------------------------------------------------------------------------------------------------------------------------
def test_statement_stft_is_torch_stft():
    x = R.make_signal("sweep", 16000, seed=3).astype(np.float64)
    want = torch.stft(torch.from_numpy(x), n_fft=321, hop_length=160, window=torch.hann_window(321, periodic=True, dtype=torch.float64), center=True,
                      pad_mode="constant", return_complex=True).abs().pow(2).T.numpy()
    got = R.stft_power(x)
    assert got.shape == want.shape == (100, 161)
    assert np.abs(got - want).max() <= 1e-12 * want.max()


def test_statement_filterbank_is_transformers_slaney():
    au = pytest.importorskip("transformers.audio_utils")
    want = au.mel_filter_bank(num_frequency_bins=161, num_mel_filters=120, min_frequency=0.0, max_frequency=8000.0, sampling_rate=16000, norm="slaney", mel_scale="slaney")
    got = R.filterbank(n_fft=320)                                    # at n_fft = 320 the two frequency grids coincide
    assert got.shape == want.shape == (161, 120)
    assert np.abs(got - want).max() <= 1e-15


def test_statement_filterbank_at_321_has_no_empty_filter_but_320_has():
    """The filters below 1 kHz are 49.86 Hz wide.  Bins 50 Hz apart (n_fft 320) miss some of them; bins 16000 / 321 = 49.84 Hz apart do
    not: filter 0 holds bin 1 alone, 0.013 Hz inside its upper edge.  So at the reference's n_fft no filter is exactly empty -- the
    lowest are merely tiny -- and a feature is exactly -1.0 only through the 80 dB floor."""
    fb = R.filterbank()
    assert fb.shape == (161, 120) and (fb >= 0).all() and (fb.max(axis=0) > 0).all()
    assert np.flatnonzero(fb[:, 0]).tolist() == [1] and fb[1, 0] < 1e-3 * fb[:, 1].max()
    assert (R.filterbank(n_fft=320).max(axis=0) == 0).sum() >= 1
    x = R.make_signal("halfsilent", R.WINDOW)
    f = R.features(x)
    assert (f[460:] == -1.0).all() and f.max() == 1.0              # the silent frames sit exactly on the floor


def test_statement_matches_the_golden_values():
    with np.load(os.path.join(R.GOLDEN, "dnsmos_golden.npz")) as z:
        g = {k: z[k] for k in z.files}
    x, rate = R.read_example()
    assert rate == 16000 and len(x) == 253760
    mean, seg, feats = R.score_clip(x)
    assert np.allclose(np.round(g["example_scores"], 4), [4.1694, 4.0475, 3.9913, 3.9566, 3.7621, 3.6139], atol=0, rtol=0)
    assert seg.shape == (6,) and np.abs(seg - g["example_scores"]).max() <= 1e-9
    assert abs(mean - float(g["example_mean"])) <= 1e-9
    assert np.abs(feats[0][g["example_feature_rows"]] - g["example_features"]).max() <= 1e-9
    a = g["anchor_scores"]
    assert seg[0] > a[0] > a[1] > a[2] and a[3] < a[1]              # a MOS predictor falls with the SNR
    for kind in R.KINDS:
        assert abs(float(R.net(R.features(R.make_signal(kind, R.WINDOW))[None])[0]) - float(g[f"{kind}_score"])) <= 1e-9


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from audiocodecs_amd.dnsmos import load_weights

    return load_weights(os.path.join(R.GOLDEN, "dnsmos_p808.npz"))


def test_argument_refusals_need_no_gpu(weights):
    from audiocodecs_amd import DNSMOS, _native, dnsmos, dnsmos_net

    sig = torch.zeros(2, 4000)
    for bad in (dict(sig=torch.zeros(4000)), dict(sample_rate=16000.0), dict(sample_rate=0), dict(sample_rate=True), dict(weights=None), dict(weights=3),
                dict(lens=torch.ones(3)), dict(lens=[1.0, 1.0]), dict(sig=torch.zeros(2, 0))):
        kw = dict(sig=sig, sample_rate=16000, weights=weights)
        kw.update(bad)
        with pytest.raises(ValueError):
            dnsmos(**kw)
    with pytest.raises(ValueError, match="no window"):
        dnsmos(sig, 16000, weights, lens=torch.tensor([1.0, 0.0]))      # a clip of length 0 after truncation
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        dnsmos(sig, 16000, weights)
    with pytest.raises(_native.NativeError, match="no CPU fallback"):
        dnsmos_net(torch.zeros(1, 16, 16), weights)
    for shape in ((16, 16), (1, 7, 16), (1, 16, 7), (1, 5000, 16)):
        with pytest.raises(ValueError):
            dnsmos_net(torch.zeros(shape), weights)
    out = dnsmos(torch.zeros(0, 4000), 16000, weights, return_segments=True)
    assert out[0].shape == (0,) and out[1].shape == (0, 0) and out[2].shape == (0, 900, 120)
    assert dnsmos_net(torch.zeros(0, 16, 16), weights).shape == (0,)
    with pytest.raises(ValueError, match="tools/make_dnsmos_golden.py"):
        DNSMOS(16000)
    met = DNSMOS(16000, model=weights)
    with pytest.raises(ValueError):
        met.append(["a"], sig)


def test_library_refusals_need_no_gpu():
    from audiocodecs_amd import _native

    L = _native.lib()
    assert L.ac_dnsmos_weights_count() == 54945 and L.ac_dnsmos_source_count() == 2 * 321 + 161 * 120
    assert L.ac_dnsmos_workspace_bytes(0, 900, 120) == 0 and L.ac_dnsmos_workspace_bytes(1, 7, 120) == 0 and L.ac_dnsmos_workspace_bytes(1, 900, 7) == 0
    one, many = L.ac_dnsmos_workspace_bytes(32, 900, 120), L.ac_dnsmos_workspace_bytes(4096, 900, 120)
    assert 0 < one < 200 << 20 and 0 < many - one <= (4096 - 32) * 4 + 256           # bounded: windows are walked in chunks, only the scores grow
    src = np.zeros(L.ac_dnsmos_source_count())
    assert L.ac_dnsmos_source(None, src.size) == -1 and L.ac_dnsmos_source(src.ctypes.data, src.size - 1) == -3
    assert L.ac_dnsmos_source(src.ctypes.data, src.size) == 0
    fb = src[642:].reshape(161, 120)
    assert np.abs(fb - R.filterbank()).max() <= 1e-15                                 # the library's filterbank is the statement's
    n = np.arange(321)
    assert np.abs(src[:321] - np.cos(2 * np.pi * n / 321)).max() <= 1e-15 and np.abs(src[321:642] - np.sin(2 * np.pi * n / 321)).max() <= 1e-15
    assert L.ac_dnsmos_net(None, 1, 16, 16, None, None, None, None, None, None, None, None, 0, None) == -1
    assert L.ac_dnsmos(None, 1, 16000, None, 1, 1, None, None, None, None, None, None, 0, None) == -1
