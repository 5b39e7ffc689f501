"""GPU tests of the fused DNSMOS (audiocodecs_amd.dnsmos, csrc/dnsmos.h) against the fp64 statement of tests/dnsmos_ref.py.

Tolerances are MEASURED, not fixed: per quantity (each stored layer, the 64 maxima, the window score, the features, the clip score) the
largest absolute error of the same statement run in float32 against fp64 over the same cases; the kernel gets 4 x that (split16 drops the
lo lo term, 2^-22 of a product where fp32 rounds at 2^-24; nothing else in the chain is looser than fp32).  The front-end cases assert on
the CPU, before the device is called, that no mel value lies within 1e-3 dB of the 80 dB floor (fp32 rounding of a mel value is about
1e-5 dB), so which values the floor takes is not a draw.  Independence of company, repetition and graph replay ask for identical bits.

The net's sweep sizes: 8 x 8 (one tile, every pool down to 1 x 1), 9 x 15 and 17 x 33 (odd at every pool: a dropped last row and column,
a tile plus one), 16 x 16, 31 x 30, 64 x 120, 225 x 30 (the third pool drops row 225's partner) and the real 900 x 120.  Figures of the
run that DESIGN.md section 8l quotes are in the parity record (`dnsmos/...`).

The module's name sorts it behind every other GPU module on purpose.  tests/test_mimi_sessions_gpu.py::test_abi_refusals_leave_everything_usable
expects a freshly allocated buffer to be refused as "a state never reset", but the library knows the states it reset by their ADDRESS
(include/audiocodecs_amd.h: memory reused at a reset state's address passes as that state), so what that test sees depends on which blocks
torch's caching allocator holds free, i.e. on every GPU module that ran before it: it passes alone, and fails behind this module or behind
tests/test_stoi_gpu.py alone.  Run last, this module leaves the allocator history of all the others as it was."""
import functools
import os

import numpy as np
import pytest
import torch

import dnsmos_ref as R
import parity_record

pytestmark = pytest.mark.gpu

SIZES = [(8, 8), (9, 15), (16, 16), (17, 33), (31, 30), (64, 120), (225, 30), (900, 120)]
NET_SWEEP = [(H, W, S) for H, W in SIZES for S in (1, 3)]
QUANTITIES = ("layer1", "layer2", "layer3", "layer4", "vec", "score")
CALL_LENGTHS = [4000, 144159, 144160, 176000, 288000]
FACTOR = 4.0
MIN_MARGIN_DB = 1e-3


@pytest.fixture(scope="module")
def weights():
    from audiocodecs_amd.dnsmos import load_weights

    return load_weights(os.path.join(R.GOLDEN, "dnsmos_p808.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def err(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max())


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- the net ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def net_case(H, W, S):
    """(feats fp32 [S, H, W] in [-1, 1], fp64 outputs, fp32 outputs) of a sweep case: computed once, read-only."""
    rng = np.random.default_rng(100000 * S + 1000 * H + W)
    feats = rng.uniform(-1.0, 1.0, (S, H, W)).astype(np.float32)
    feats.setflags(write=False)

    def flat(out):
        score, layers, vec = out
        return dict(zip(QUANTITIES, [*layers, vec, score]))

    return feats, flat(R.net(feats, return_layers=True)), flat(R.net(feats, dtype=torch.float32, return_layers=True))


@pytest.fixture(scope="module")
def net_tol():
    """Per quantity the fp32 statement's largest error against fp64 over the sweep, times FACTOR."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for H, W, S in NET_SWEEP:
        _, d64, d32 = net_case(H, W, S)
        for q in QUANTITIES:
            worst[q] = max(worst[q], err(d32[q], d64[q]))
    return {q: FACTOR * v for q, v in worst.items()}, worst


@pytest.mark.parametrize("H,W,S", NET_SWEEP)
def test_net_sweep(weights, net_tol, H, W, S):
    from audiocodecs_amd import dnsmos_net

    tol, fp32 = net_tol
    feats, want, _ = net_case(H, W, S)
    score, layers, vec = dnsmos_net(dev(feats), weights, return_layers=True)
    torch.cuda.synchronize()
    got = dict(zip(QUANTITIES, [*(t.cpu().numpy() for t in layers), vec.cpu().numpy(), score.cpu().numpy()]))
    errs = {}
    for q in QUANTITIES:
        assert got[q].shape == want[q].shape and got[q].dtype == np.float32, q
        errs[q] = err(got[q], want[q])
    print(f"dnsmos net H={H} W={W} S={S}: " + ", ".join(f"{q} {errs[q]:.3e} (fp32 {fp32[q]:.3e}, tol {tol[q]:.3e})" for q in QUANTITIES))
    parity_record.record("dnsmos", f"net/H{H}_W{W}_S{S}", **{f"kernel_{q}_err": errs[q] for q in QUANTITIES}, **{f"{q}_tol": tol[q] for q in QUANTITIES})
    assert torch.equal(dnsmos_net(dev(feats), weights), score), "without return_layers"
    for q in QUANTITIES:
        assert errs[q] <= tol[q], (q, errs[q], tol[q])


def test_net_window_does_not_depend_on_its_company(weights):
    from audiocodecs_amd import dnsmos_net

    feats = dev(net_case(64, 120, 3)[0])
    whole = dnsmos_net(feats, weights, return_layers=True)
    again = dnsmos_net(feats, weights, return_layers=True)
    alone = dnsmos_net(feats[1:2], weights, return_layers=True)
    for a, b, c in zip([whole[0], *whole[1], whole[2]], [again[0], *again[1], again[2]], [alone[0], *alone[1], alone[2]]):
        assert np.array_equal(bits(a), bits(b)), "two runs"
        assert np.array_equal(bits(a[1:2]), bits(c)), "window 1 alone"


# ---- the front end ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def window_case(kind):
    x = R.make_signal(kind, R.WINDOW)
    x.setflags(write=False)
    return x, R.features(x), R.features(x, np.float32)


@pytest.fixture(scope="module")
def feat_tol():
    worst = max(err(window_case(k)[2], window_case(k)[1]) for k in R.KINDS)
    return FACTOR * worst, worst


@pytest.mark.parametrize("kind", R.KINDS)
def test_front_end(weights, feat_tol, kind):
    from audiocodecs_amd import dnsmos

    tol, fp32 = feat_tol
    x, want, _ = window_case(kind)
    margin = R.floor_margin_db(x)
    assert margin >= MIN_MARGIN_DB, f"a mel value lies {margin:.2e} dB from the 80 dB floor: the floor of this case would be a draw"
    score, segs, feats = dnsmos(dev(x[None]), 16000, weights, return_segments=True)
    torch.cuda.synchronize()
    assert feats.shape == (1, 900, 120) and segs.shape == (1, 1) and feats.dtype == torch.float32
    got = feats[0].cpu().numpy()
    e = err(got, want)
    print(f"dnsmos front end {kind}: features {e:.3e} (fp32 statement {fp32:.3e}, tolerance {tol:.3e}); margin {margin:.3f} dB; {(want == -1.0).sum()} values on the floor")
    parity_record.record("dnsmos", f"front/{kind}", kernel_feature_err=e, fp32_feature_err=fp32, feature_tol=tol, margin_db=margin)
    assert got.max() == 1.0 and got.min() >= -1.0
    assert np.array_equal(got == -1.0, want == -1.0), "the 80 dB floor takes other values than the statement's"
    if kind == "halfsilent":
        assert (got[460:] == -1.0).all()                             # silent frames: mel power exactly 0, exactly on the floor
    for m in np.flatnonzero(R.filterbank().max(axis=0) == 0.0):      # an empty filter is exactly -1.0 (at n_fft 321 there is none: test_dnsmos_cpu.py)
        assert (got[:, m] == -1.0).all()
    assert e <= tol


# ---- the whole call ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_case(L16, kind="noise"):
    x = R.make_signal(kind, L16, seed=L16 % 7)
    x.setflags(write=False)
    return x, R.score_clip(x), R.score_clip(x, np.float32)


@pytest.fixture(scope="module")
def call_tol():
    """(clip score, window score) tolerances over the whole-call cases, the example clip included."""
    worst = [0.0, 0.0]
    cases = [clip_case(L) for L in CALL_LENGTHS] + [example_case()]
    for _, d64, d32 in cases:
        worst = [max(worst[0], abs(d32[0] - d64[0])), max(worst[1], err(d32[1], d64[1]))]
    return [FACTOR * v for v in worst], worst


@functools.lru_cache(maxsize=None)
def example_case():
    x, rate = R.read_example()
    assert rate == 16000
    x.setflags(write=False)
    return x, R.score_clip(x), R.score_clip(x, np.float32)


@pytest.mark.parametrize("L16", CALL_LENGTHS)
def test_whole_call(weights, call_tol, L16):
    from audiocodecs_amd import dnsmos, dnsmos_segments

    tol, fp32 = call_tol
    x, (mean, seg, _), _ = clip_case(L16)
    n = len(dnsmos_segments(L16))
    assert n == len(seg)
    score, segs, feats = dnsmos(dev(x[None]), 16000, weights, return_segments=True)
    torch.cuda.synchronize()
    assert score.shape == (1,) and segs.shape == (1, n) and feats.shape == (n, 900, 120) and score.dtype == torch.float32
    e = [abs(float(score[0]) - mean), err(segs[0].cpu().numpy(), seg)]
    print(f"dnsmos call L16={L16}: {n} windows, clip {e[0]:.3e} (fp32 {fp32[0]:.3e}, tol {tol[0]:.3e}), window {e[1]:.3e} (fp32 {fp32[1]:.3e}, tol {tol[1]:.3e})")
    parity_record.record("dnsmos", f"call/L{L16}", windows=n, kernel_clip_err=e[0], kernel_window_err=e[1], clip_tol=tol[0], window_tol=tol[1])
    assert torch.equal(dnsmos(dev(x[None]), 16000, weights), score), "without return_segments"
    assert e[0] <= tol[0] and e[1] <= tol[1]


def test_whole_call_honours_lens(weights, call_tol):
    from audiocodecs_amd import dnsmos

    tol, _ = call_tol
    L = 288000
    x = np.stack([clip_case(L)[0], clip_case(L)[0], clip_case(L)[0]])
    lens = torch.tensor([1.0, 0.5, 1.0 / 64.0], dtype=torch.float32)
    cut = [int(np.float64(v) * L) for v in lens.numpy()]
    assert cut == [288000, 144000, 4500]                             # (144000 is doubled once, 4500 six times)
    score, segs, _ = dnsmos(dev(x), 16000, weights, lens=lens.cuda(), return_segments=True)
    torch.cuda.synchronize()
    counts = [len(R.reference_windows(x[b][:cut[b]])) for b in range(3)]
    assert segs.shape == (3, max(counts))
    for b in range(3):
        mean, seg, _ = R.score_clip(x[b][:cut[b]])
        row = segs[b].cpu().numpy()
        assert np.isnan(row[counts[b]:]).all() and not np.isnan(row[:counts[b]]).any()
        assert abs(float(score[b]) - mean) <= tol[0] and err(row[:counts[b]], seg) <= tol[1]
    assert np.array_equal(bits(score[0:1]), bits(dnsmos(dev(x[0:1]), 16000, weights))), "lens = 1 is no lens"


def test_whole_call_from_24_khz(weights, call_tol):
    from audiocodecs_amd import dnsmos
    from audiocodecs_amd.resample import resample

    tol, _ = call_tol
    x = dev(R.make_signal("noise", 24000 * 10, seed=4)[None])
    score, segs, feats = dnsmos(x, 24000, weights, return_segments=True)
    x16 = resample(x, 24000, 16000)
    assert x16.shape == (1, 160000) and segs.shape == (1, 1)
    again = dnsmos(x16, 16000, weights, return_segments=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip((score, segs, feats), again))
    mean, seg, _ = R.score_clip(x16[0].cpu().numpy())
    parity_record.record("dnsmos", "call/resampled_24k", kernel_clip_err=abs(float(score[0]) - mean), clip_tol=tol[0])
    assert abs(float(score[0]) - mean) <= tol[0]


def test_example_clip(weights, call_tol):
    from audiocodecs_amd import dnsmos

    tol, fp32 = call_tol
    x, (mean, seg, _), _ = example_case()
    score, segs, _ = dnsmos(dev(x[None]), 16000, weights, return_segments=True)
    got = segs[0].cpu().numpy()
    e = [abs(float(score[0]) - mean), err(got, seg)]
    print(f"dnsmos example clip: windows {np.round(got, 4)}, clip {e[0]:.3e} (tol {tol[0]:.3e}), window {e[1]:.3e} (tol {tol[1]:.3e})")
    parity_record.record("dnsmos", "call/example", kernel_clip_err=e[0], kernel_window_err=e[1], fp32_clip_err=fp32[0], fp32_window_err=fp32[1], clip_tol=tol[0], window_tol=tol[1])
    assert err(got, np.array([4.1694, 4.0475, 3.9913, 3.9566, 3.7621, 3.6139])) <= 1e-4        # the figures as quoted to four decimals (half a unit is 5e-5)
    assert e[0] <= tol[0] and e[1] <= tol[1]


# ---- identity of bits -------------------------------------------------------------------------------------------------------------------
def test_a_clip_does_not_depend_on_its_company(weights):
    from audiocodecs_amd import dnsmos

    L = 176000
    x = np.stack([R.make_signal(k, L, seed=1) for k in R.KINDS])
    whole = dnsmos(dev(x), 16000, weights, return_segments=True)
    again = dnsmos(dev(x), 16000, weights, return_segments=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(whole, again)), "two runs"
    alone = dnsmos(dev(x[1:2]), 16000, weights, return_segments=True)
    n = alone[2].shape[0]
    assert np.array_equal(bits(whole[0][1:2]), bits(alone[0])) and np.array_equal(bits(whole[1][1:2]), bits(alone[1]))
    assert np.array_equal(bits(whole[2][n:2 * n]), bits(alone[2]))


def test_replays_from_a_captured_graph(weights):
    from audiocodecs_amd import dnsmos

    L = 150000
    a, b = (R.make_signal(k, L, seed=2)[None] for k in ("noise", "sweep"))
    sig = dev(np.concatenate([a, b]))
    eager = dnsmos(sig, 16000, weights)                                # (also builds the tables, the packed weights and the plan: a capture cannot)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = dnsmos(sig, 16000, weights)
    torch.cuda.current_stream().wait_stream(side)
    for data, want in ((np.concatenate([a, b]), eager), (np.concatenate([b, a]), None), (np.concatenate([a, b]), eager)):
        sig.copy_(dev(data))
        g.replay()
        torch.cuda.synchronize()
        if want is None:
            want = dnsmos(dev(data), 16000, weights)
        assert np.array_equal(bits(out), bits(want))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_bad_sample_spoils_its_clip_only(weights, bad):
    from audiocodecs_amd import dnsmos

    L = 150000
    x = np.stack([R.make_signal("noise", L, seed=s) for s in (5, 6, 7)])
    clean = dnsmos(dev(x), 16000, weights)
    for where in (0, L // 2, 143999):
        y = x.copy()
        y[1, where] = bad
        got = dnsmos(dev(y), 16000, weights)
        assert bool(torch.isnan(got[1])), where
        assert np.array_equal(bits(got[[0, 2]]), bits(clean[[0, 2]])), where


# ---- wrappers ---------------------------------------------------------------------------------------------------------------------------
def test_metric_class_on_the_device(weights):
    from audiocodecs_amd import DNSMOS, dnsmos

    x = dev(np.stack([R.make_signal("noise", 24000, seed=8), R.make_signal("sweep", 24000, seed=8)]))
    lens = torch.tensor([1.0, 0.5])
    want = dnsmos(x, 24000, weights, lens=lens)
    met = DNSMOS(24000, model=os.path.join(R.GOLDEN, "dnsmos_p808.npz"))
    met.append(["x", "y"], x, lens=lens)
    assert met.ids == ["x", "y"] and met.scores == want.cpu().tolist()
    assert met.summarize("average") == pytest.approx(float(want.double().mean()))
    assert not torch.equal(want, dnsmos(x, 24000, weights))            # `lens` is honoured


def test_resynthesis_dnsmos_is_the_chain_of_public_calls(weights, checkpoints):
    from audiocodecs_amd import Encodec, dnsmos

    cfg, sd = checkpoints("tiny", 0)
    codec = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    sig = dev(np.stack([R.make_signal("noise", 12001, seed=9), R.make_signal("sweep", 12001, seed=9)]))
    score = codec.resynthesis_dnsmos(sig, weights)
    assert score.shape == (2,) and score.dtype == torch.float32 and bool(torch.isfinite(score).all())
    rec = codec.toks_to_sig(codec.sig_to_toks(sig))
    T = sig.shape[-1]
    rec = torch.nn.functional.pad(rec, [0, T - rec.shape[-1]], mode="replicate") if rec.shape[-1] < T else rec.narrow(-1, 0, T)
    assert torch.equal(score, dnsmos(rec, 24000, weights))
    parity_record.record("dnsmos", "resynthesis/encodec_tiny", dnsmos=float(score.mean()))
