"""GPU tests of `Codec.resynthesis_report`: one encode and one decode give what the three `resynthesis_*` methods give with three of each.

A tiny EnCodec with seeded random weights, three clips of about a second (24001 samples: the decode is longer than the input, so the length
adjustment is exercised).  The existing methods are run twice first: they are bitwise repeatable on these inputs, so the report is held to
`torch.equal`."""
import os

import numpy as np
import pytest
import torch

import tokstats_ref as R

pytestmark = pytest.mark.gpu

RATE = 24000
T = 24001


@pytest.fixture(scope="module")
def codec(checkpoints):
    from audiocodecs_amd import Encodec

    cfg, sd = checkpoints("tiny", 0)
    return Encodec(RATE, num_codebooks=8, state_dict=sd, config=cfg).eval(), cfg


@pytest.fixture(scope="module")
def sig():
    rng = np.random.default_rng(77)
    t = np.arange(T) / RATE
    clips = [0.1 * rng.standard_normal(T), 0.3 * np.sin(2 * np.pi * (200 + 900 * t) * t), 0.05 * rng.standard_normal(T) + 0.2 * np.sin(2 * np.pi * 440 * t)]
    return torch.from_numpy(np.stack(clips).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def weights():
    from audiocodecs_amd.dnsmos import load_weights

    return load_weights(os.path.join(R.GOLDEN, "dnsmos_p808.npz"))


class Counted:
    """Counts the calls of two public methods of ONE instance (the class and every other instance stay as they are)."""

    def __init__(self, codec):
        self.codec, self.calls = codec, {"sig_to_toks": 0, "toks_to_sig": 0}

    def __enter__(self):
        for name in self.calls:
            def wrapper(*args, _name=name, _fn=getattr(self.codec, name), **kwargs):
                self.calls[_name] += 1
                return _fn(*args, **kwargs)

            self.codec.__dict__[name] = wrapper
        return self.calls

    def __exit__(self, *exc):
        for name in self.calls:
            del self.codec.__dict__[name]


def test_report_equals_the_three_methods_with_one_encode_and_one_decode(codec, sig, weights):
    from audiocodecs_amd import CodebookUtil

    codec, cfg = codec
    first = (*codec.resynthesis_distances(sig), codec.resynthesis_stoi(sig), codec.resynthesis_dnsmos(sig, weights))
    again = (*codec.resynthesis_distances(sig), codec.resynthesis_stoi(sig), codec.resynthesis_dnsmos(sig, weights))
    for name, a, b in zip(("stft", "mel", "stoi", "dnsmos"), first, again):
        spread = float((a.double() - b.double()).abs().max())
        print(f"resynthesis_{name}: spread between two runs {spread:.3e}")
        assert torch.equal(a, b), f"{name}: two runs of the existing method differ by {spread:.3e}"
    toks = codec.sig_to_toks(sig)
    metric = CodebookUtil(8, cfg.codebook_size)
    with Counted(codec) as calls:
        report = codec.resynthesis_report(sig, dnsmos_weights=weights, codebook_util=metric)
    assert calls == {"sig_to_toks": 1, "toks_to_sig": 1}
    assert set(report) == {"toks", "stft", "mel", "stoi", "dnsmos"}
    assert torch.equal(report["toks"], toks) and toks.shape[0] == 3 and toks.shape[2] == 8
    for name, want in zip(("stft", "mel", "stoi", "dnsmos"), first):
        assert report[name].shape == (3,) and bool(torch.isfinite(report[name]).all())
        assert torch.equal(report[name], want), (name, report[name], want)
    assert torch.equal(metric.state.counts.cpu(), R.histogram(toks, cfg.codebook_size))
    assert int(metric.state.total) == toks.shape[0] * toks.shape[1] and int(metric.state.bad) == 0
    want = R.summary64(metric.state.counts.cpu())
    assert metric.summarize() == want


def test_report_without_weights_and_with_lengths(codec, sig):
    from audiocodecs_amd import CodebookUtil

    codec, cfg = codec
    length = torch.tensor([1.0, 0.6, 0.8], device="cuda")       # (times 75 or 76 frames: at least 0.2 from a half-integer)
    stft, mel = codec.resynthesis_distances(sig, length)
    stoi = codec.resynthesis_stoi(sig, length)
    toks = codec.sig_to_toks(sig, length)
    metric = CodebookUtil(8, cfg.codebook_size)
    with Counted(codec) as calls:
        report = codec.resynthesis_report(sig, length, codebook_util=metric)
        assert calls == {"sig_to_toks": 1, "toks_to_sig": 1}
        codec.resynthesis_report(sig, length)
        assert calls == {"sig_to_toks": 2, "toks_to_sig": 2}
    assert set(report) == {"toks", "stft", "mel", "stoi"}
    assert torch.equal(report["toks"], toks) and torch.equal(report["stft"], stft) and torch.equal(report["mel"], mel) and torch.equal(report["stoi"], stoi)
    N = toks.shape[1]
    prod = length.double().cpu() * N
    nvalid = prod.round().clamp(0, N).long()
    assert torch.equal(metric.state.counts.cpu(), R.histogram(toks, cfg.codebook_size, nvalid)) and int(metric.state.total) == int(nvalid.sum())
    with pytest.raises(ValueError):
        codec.resynthesis_report(sig[0])
