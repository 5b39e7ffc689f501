"""GPU tests of the fused spectral distances (audiocodecs_amd.metrics, csrc/specdist.h) against the fp64 statement of
tests/specdist_ref.py.  The tolerance is MEASURED, not fixed: per signal kind, the largest relative error of the reference's own fp32
arithmetic (torch.stft, fp32 matmul, log10, on the CPU) against the fp64 statement over that kind's sweep cases, per clip and per frame
separately; the kernel gets 4 x that (split16 drops the lo lo term, 2^-22 of a product where fp32 rounds at 2^-24; nothing else in the
chain is looser than fp32).  Identity, symmetry, independence and graph replay ask for identical bits.

Figures of the run that DESIGN.md section 8j quotes are in the parity record (`specdist/...`)."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity_record
import specdist_ref as R

pytestmark = pytest.mark.gpu

# the kernel's frame tile is 16: F = 2, 3 (one partial tile), 16 (a full tile), 17 (a seam, a tile of one frame), 34, 51 (partial last tiles)
LENGTHS = [513, 640, 5119, 5120, 5121, 10560, 16000]
FRAMES = [2, 3, 16, 17, 17, 34, 51]
# The full cross product, the kinds cycling through it: 28 cases, 9 or 10 per kind.  Not fewer: the tolerance of a kind is the LARGEST fp32
# error over its cases, and that error has a heavy tail -- the frame that reflect padding makes symmetric about its centre (frame 0) has
# a spectrum that is real up to a phase and changes sign between bins, so one bin of it usually lies 5 to 6 decades below the frame's
# peak, at the rounding floor of ANY fp32 arithmetic, and what that bin's dB comes to is a draw, for the reference as for the kernel.
# The largest of many draws is a steadier yardstick than the largest of four.
SWEEP = [(L, B, P, R.KINDS[(i + j + k) % 3]) for i, L in enumerate(LENGTHS) for j, B in enumerate((1, 3)) for k, P in enumerate((1, 3))]
FACTOR = 4.0


def case_data(L, B, P, kind):
    """(hyp [P, B, L], ref [B, L]) of a sweep case."""
    seed = 17 * L + 5 * B + P
    pairs = [R.make_pair(kind, seed, B, L, hyp=p) for p in range(P)]
    return np.stack([h for h, _ in pairs]), pairs[0][1]


class Sweep:
    """Computed once: per sweep case the fp64 distances and the fp32 reference's, and from those the tolerance of every kind."""

    def __init__(self):
        self.want, self.fp32_err = {}, {k: [0.0, 0.0] for k in R.KINDS}
        for case in SWEEP:
            L, B, P, kind = case
            hyp, ref = case_data(*case)
            self.want[case] = [R.distances(hyp[p], ref) for p in range(P)]
            for p in range(P):
                got, want = R.torch_fp32(hyp[p], ref), self.want[case][p]
                clip = max(R.rel_err(got[0], want[0]), R.rel_err(got[1], want[1]))
                frame = max(R.rel_err(got[2], want[2]), R.rel_err(got[3], want[3]))
                self.fp32_err[kind] = [max(self.fp32_err[kind][0], clip), max(self.fp32_err[kind][1], frame)]
        self.kernel_err = {k: [0.0, 0.0] for k in R.KINDS}

    def tol(self, kind):
        return FACTOR * self.fp32_err[kind][0], FACTOR * self.fp32_err[kind][1]


@pytest.fixture(scope="module")
def sweep():
    return Sweep()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(hyp, ref, sample_rate=16000):
    from audiocodecs_amd import spectral_distances

    out = spectral_distances(dev(hyp), dev(ref), sample_rate, return_frames=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


def errors(got, want):
    """(per-clip, per-frame) largest relative error of one hypothesis' four results against the fp64 statement."""
    return max(R.rel_err(got[0], want[0]), R.rel_err(got[1], want[1])), max(R.rel_err(got[2], want[2]), R.rel_err(got[3], want[3]))


def test_sweep_covers_every_length_count_and_kind():
    assert [1 + L // 320 for L in LENGTHS] == FRAMES
    assert {c[0] for c in SWEEP} == set(LENGTHS) and {c[1] for c in SWEEP} == {1, 3} and {c[2] for c in SWEEP} == {1, 3} and {c[3] for c in SWEEP} == set(R.KINDS)
    for kind in R.KINDS:
        assert {c[0] for c in SWEEP if c[3] == kind} >= {513, 16000} and len([c for c in SWEEP if c[3] == kind]) >= 9


@pytest.mark.parametrize("L,B,P,kind", SWEEP)
def test_shape_sweep(sweep, L, B, P, kind):
    hyp, ref = case_data(L, B, P, kind)
    got = run(hyp if P > 1 else hyp[0], ref)
    lead = (P,) if P > 1 else ()
    assert got[0].shape == lead + (B,) and got[1].shape == lead + (B,) and got[2].shape == lead + (B, 1 + L // 320) and got[3].shape == got[2].shape
    assert all(g.dtype == np.float32 for g in got)
    clip = frame = 0.0
    for p in range(P):
        c, f = errors([g[p] if P > 1 else g for g in got], sweep.want[(L, B, P, kind)][p])
        clip, frame = max(clip, c), max(frame, f)
    tol = sweep.tol(kind)
    sweep.kernel_err[kind] = [max(sweep.kernel_err[kind][0], clip), max(sweep.kernel_err[kind][1], frame)]
    print(f"specdist sweep L={L} B={B} P={P} {kind}: kernel clip {clip:.3e} frame {frame:.3e}; fp32 reference (kind's worst) clip {sweep.fp32_err[kind][0]:.3e} "
          f"frame {sweep.fp32_err[kind][1]:.3e}; tolerance clip {tol[0]:.3e} frame {tol[1]:.3e}")
    parity_record.record("specdist", f"sweep/L{L}_B{B}_P{P}_{kind}", kernel_clip_err=clip, kernel_frame_err=frame, fp32_clip_err=sweep.fp32_err[kind][0],
                         fp32_frame_err=sweep.fp32_err[kind][1], clip_tol=tol[0], frame_tol=tol[1])
    assert clip <= tol[0] and frame <= tol[1]


def test_identical_signals_give_exactly_zero():
    ref = R.make_signal("floor", 2, 3, 5121)
    for g in run(ref, ref) + run(np.stack([ref, ref, ref]), ref):
        assert (g.view(np.uint32) == 0).all()


def test_swapping_hypothesis_and_reference_returns_the_same_bits():
    hyp, ref = R.make_pair("dynamic", 4, 3, 10560)
    assert same_bits(run(hyp, ref), run(ref, hyp))


def test_gain_of_two(sweep):
    ref = R.make_signal("floor", 5, 2, 5121)
    got = run(2.0 * ref, ref)
    s, m = 10 * np.log10(2.0) * np.sqrt(513), 10 * np.log10(2.0) * np.sqrt(80)
    clip = max(R.rel_err(got[0], s), R.rel_err(got[1], m))
    frame = max(R.rel_err(got[2], s), R.rel_err(got[3], m))
    tol = sweep.tol("floor")
    print(f"specdist gain: clip {clip:.3e} frame {frame:.3e}; tolerance {tol[0]:.3e} {tol[1]:.3e}")
    parity_record.record("specdist", "gain_of_two", kernel_clip_err=clip, kernel_frame_err=frame, clip_tol=tol[0], frame_tol=tol[1])
    assert clip <= tol[0] and frame <= tol[1]


def test_a_clip_does_not_depend_on_its_company():
    from audiocodecs_amd import spectral_distances

    L = 5121
    pairs = [R.make_pair("noise", 6, 3, L, hyp=p) for p in range(3)]
    hyp, ref = np.stack([h for h, _ in pairs]), pairs[0][1]
    whole = run(hyp, ref)                                   # [3, 3, ...]
    assert same_bits(whole, run(hyp, ref)), "two runs"
    for p in range(3):
        one = run(hyp[p], ref)                              # P separate calls
        assert same_bits([g[p] for g in whole], one), f"hypothesis {p} alone"
    alone = run(hyp[1, 2:3], ref[2:3])                      # B = 1
    assert same_bits([g[1, 2:3] for g in whole], alone), "clip 2 alone"
    d_h, d_r = dev(hyp), dev(ref)
    view = spectral_distances(d_h[1, 2:3], d_r[2:3], 16000, return_frames=True)      # a row of the larger batch as it stands
    assert same_bits([g[1, 2:3] for g in whole], [t.cpu().numpy() for t in view])


def test_replays_from_a_captured_graph():
    from audiocodecs_amd import spectral_distances

    hyp, ref = R.make_pair("floor", 8, 3, 10560)
    sh, sr = dev(hyp), dev(ref)
    eager = spectral_distances(sh, sr, 16000, return_frames=True)       # (also builds the tables: a capture cannot)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            so = spectral_distances(sh, sr, 16000, return_frames=True)
    torch.cuda.current_stream().wait_stream(side)
    hyp2 = R.make_pair("floor", 8, 3, 10560, hyp=1)[0]
    for data, want in ((hyp, eager), (hyp2, None), (hyp, eager)):
        sh.copy_(dev(data))
        g.replay()
        torch.cuda.synchronize()
        if want is None:
            want = spectral_distances(dev(data), sr, 16000, return_frames=True)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(so, want))


def test_tile_scaling_keeps_the_quiet_half(sweep):
    """The `dynamic` kind's second half lies 2^-14 below its first: its frames must meet the per-frame tolerance the loud frames meet
    (a scale taken per clip would leave them 14 bits short)."""
    L = 16000
    hyp, ref = R.make_pair("dynamic", 9, 2, L)
    got, want = run(hyp, ref), R.distances(hyp, ref)
    quiet = np.arange(1 + L // 320) * 320 - 512 >= L // 2          # frames that lie wholly in the quiet half
    assert quiet.sum() >= 20 and (~quiet).sum() >= 20
    tol = sweep.tol("dynamic")[1]
    errs = {}
    for name, sel in (("loud", ~quiet), ("quiet", quiet)):
        errs[name] = max(R.rel_err(got[2][:, sel], want[2][:, sel]), R.rel_err(got[3][:, sel], want[3][:, sel]))
    print(f"specdist tile scaling: loud frames {errs['loud']:.3e}, quiet frames {errs['quiet']:.3e}; tolerance {tol:.3e}")
    parity_record.record("specdist", "tile_scaling", loud_frame_err=errs["loud"], quiet_frame_err=errs["quiet"], frame_tol=tol)
    assert errs["loud"] <= tol and errs["quiet"] <= tol


def test_resampled_path(sweep):
    from audiocodecs_amd.resample import resample

    hyp, ref = R.make_pair("floor", 10, 2, 24000)
    got = run(hyp, ref, 24000)
    h16, r16 = (resample(dev(x), 24000, 16000).cpu().numpy() for x in (hyp, ref))
    assert h16.shape == (2, 16000) and got[2].shape == (2, 51)
    clip, frame = errors(got, R.distances(h16, r16))
    tol = sweep.tol("floor")
    parity_record.record("specdist", "resampled_24k", kernel_clip_err=clip, kernel_frame_err=frame, clip_tol=tol[0], frame_tol=tol[1])
    assert clip <= tol[0] and frame <= tol[1]
    assert same_bits(got, run(h16, r16))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_bad_sample_spoils_its_clip_only(bad):
    hyp, ref = R.make_pair("noise", 11, 3, 5121)
    clean = run(hyp, ref)
    for where, side in ((2000, "hyp"), (0, "ref"), (5120, "hyp")):
        h, r = hyp.copy(), ref.copy()
        (h if side == "hyp" else r)[1, where] = bad
        got = run(h, r)
        assert np.isnan(got[0][1]) and np.isnan(got[1][1]), (where, side)
        assert same_bits([g[[0, 2]] for g in got], [g[[0, 2]] for g in clean])
        touched = np.abs(np.arange(17) * 320 - where) < 512 + (where == 0)       # frames whose window holds the sample (reflected at the edges)
        assert np.isnan(got[2][1][touched]).all() and np.isnan(got[3][1][touched]).all()


def test_abi_refusals_launch_nothing():
    from audiocodecs_amd import _native, metrics

    lib = _native.lib()
    P, B, L = 1, 2, 5121
    hyp, ref = (dev(a) for a in R.make_pair("noise", 12, B, L))
    tables = metrics._host.tables("specdist", hyp.device)
    nws = lib.ac_specdist_workspace_bytes(P, B, L)
    ws = torch.zeros(nws + 16, dtype=torch.uint8, device="cuda")
    so, mo = torch.full((B,), 7.0, device="cuda"), torch.full((B,), 7.0, device="cuda")
    p = lambda x, o=0: C.c_void_p(x.data_ptr() + o)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = lambda **kw: [kw.get("hyp", p(hyp)), kw.get("ref", p(ref)), kw.get("P", P), B, kw.get("L", L), kw.get("tab", p(tables)), kw.get("so", p(so)), p(mo), None, None,
                         kw.get("ws", p(ws)), kw.get("nws", nws), st]
    for kw in (dict(hyp=None), dict(ref=None), dict(tab=None), dict(so=None), dict(ws=None), dict(hyp=p(hyp, 2)), dict(tab=p(tables, 4)), dict(ws=p(ws, 8)),
               dict(L=512), dict(P=5), dict(P=0)):
        assert lib.ac_specdist(*args(**kw)) == -1, kw
    assert lib.ac_specdist(*args(nws=nws - 1)) == -3
    assert lib.ac_specdist_tables(p(tables), p(tables), lib.ac_specdist_tables_bytes() - 1, st) == -3
    torch.cuda.synchronize()
    assert (so == 7.0).all() and (mo == 7.0).all() and (ws == 0).all(), "a refused call launched"
    assert lib.ac_specdist(*args()) == 0
    torch.cuda.synchronize()
    want = run(hyp.cpu().numpy(), ref.cpu().numpy())
    assert same_bits((so.cpu().numpy(), mo.cpu().numpy()), want[:2])


def test_metric_classes_on_the_device():
    from audiocodecs_amd import MelDistance, STFTDistance

    hyp, ref = R.make_pair("floor", 13, 2, 7200)
    want = run(hyp, ref, 24000)
    sd, md = STFTDistance(24000), MelDistance(24000)
    sd.append(["x", "y"], dev(hyp), dev(ref), lens=torch.ones(2))
    md.append(["x", "y"], dev(hyp), dev(ref))
    assert sd.ids == ["x", "y"] and sd.scores == want[0].tolist() and md.scores == want[1].tolist()


def test_resynthesis_distances_is_the_chain_of_public_calls(checkpoints):
    from audiocodecs_amd import Encodec, spectral_distances

    cfg, sd = checkpoints("tiny", 0)
    codec = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    g = torch.Generator().manual_seed(5)
    sig = (torch.randn(2, 6001, generator=g) * 0.1).cuda()
    stft, mel = codec.resynthesis_distances(sig)
    assert stft.shape == (2,) and mel.shape == (2,) and bool(torch.isfinite(stft).all()) and bool(torch.isfinite(mel).all())
    rec = codec.toks_to_sig(codec.sig_to_toks(sig))
    T = sig.shape[-1]
    rec = torch.nn.functional.pad(rec, [0, T - rec.shape[-1]], mode="replicate") if rec.shape[-1] < T else rec.narrow(-1, 0, T)
    want = spectral_distances(rec, sig, 24000)
    assert torch.equal(stft, want[0]) and torch.equal(mel, want[1])
    parity_record.record("specdist", "resynthesis/encodec_tiny", stft=float(stft.mean()), mel=float(mel.mean()))
