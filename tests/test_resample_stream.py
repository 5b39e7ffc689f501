"""The stateful resampler off the GPU (audiocodecs_amd.ResampleStream, include/audiocodecs_amd.h ac_resample_stream_*).

The output-length rule of a push is pure host arithmetic in the library (ac_resample_stream_out_len): it is checked here against a
chunked numpy restatement of the polyphase FIR that knows nothing of that rule -- it keeps every sample a later output may still
read, emits an output group as soon as all its taps are in, and is itself pinned to the one-shot fp64 oracle
(oracle/resample_oracle.py).  The GPU side is tests/test_resample_stream_gpu.py."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import resample_oracle as R

RATES = [(16000, 24000), (24000, 16000), (16000, 44100), (44100, 16000)]
LENGTHS = [0, 1, 5, 17, 1001, 5003]


def schedules(L):
    """Push sizes covering L samples: one push, single samples (then the rest), and a ragged cycle with empty pushes."""
    out = {"single": [L], "one_sample": [1] * min(L, 40) + ([L - 40] if L > 40 else [])}
    ragged, done, i = [], 0, 0
    cyc = (7, 0, 213, 1, 320, 2)
    while done < L:
        n = min(cyc[i % len(cyc)], L - done)
        ragged.append(n)
        done += n
        i += 1
    out["ragged"] = ragged
    return out


class NumpyStream:
    """Chunked fp64 restatement: `held` is the input from absolute position `start` on (positions < 0 are the left padding's zeros)."""

    def __init__(self, orig, new, B):
        self.k, self.n, self.o, self.width = R.kernel(orig, new)
        self.taps = self.k.shape[1]
        self.start = -self.width
        self.held = np.zeros((B, self.width))
        self.group = 0            # next output group
        self.total = 0
        self.max_history = 0

    def _emit(self, upto_input):
        """Every group whose last tap lies before absolute input position `upto_input`."""
        out = []
        while self.group * self.o - self.width + self.taps <= upto_input:
            a = self.group * self.o - self.width - self.start
            out.append(self.held[:, a:a + self.taps] @ self.k.T)      # [B, n]
            self.group += 1
        return np.concatenate(out, 1) if out else np.zeros((self.held.shape[0], 0))

    def push(self, x):
        self.held = np.concatenate([self.held, x.astype(np.float64)], 1)
        self.total += x.shape[1]
        y = self._emit(self.total)
        drop = self.group * self.o - self.width - self.start          # nothing before the next group's first tap is read again
        drop = max(0, min(drop, self.held.shape[1]))
        self.held, self.start = self.held[:, drop:], self.start + drop
        self.max_history = max(self.max_history, self.held.shape[1])
        return y

    def finish(self):
        want = math.ceil(self.n * self.total / self.o) - self.group * self.n
        groups = -(-want // self.n)
        self.held = np.concatenate([self.held, np.zeros((self.held.shape[0], groups * self.o + self.taps))], 1)
        if groups <= 0:
            return np.zeros((self.held.shape[0], 0))
        return self._emit((self.group + groups - 1) * self.o - self.width + self.taps)[:, :want]


def _helper():
    from audiocodecs_amd import _native

    if not os.path.exists(_native.lib_path):
        import __graft_entry__

        __graft_entry__.build()
    from audiocodecs_amd.resample import stream_out_len

    return stream_out_len


@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_output_length_rule_against_the_chunked_restatement(rates):
    out_len = _helper()
    rng = np.random.default_rng(11)
    for L in LENGTHS:
        x = rng.standard_normal((2, L))
        ref = R.resample(x, *rates)
        for kind, sizes in schedules(L).items():
            s = NumpyStream(*rates, 2)
            n, o, width, taps = s.n, s.o, s.width, s.taps
            outs, consumed = [], 0
            for c in sizes:
                y = s.push(x[:, consumed:consumed + c])
                assert y.shape[1] == out_len(consumed, c, n, o, width), (rates, L, kind, consumed, c)
                assert y.shape[1] % n == 0
                consumed += c
                outs.append(y)
                assert s.max_history <= taps - 1, (rates, L, kind, s.max_history)
            tail = s.finish()
            assert tail.shape[1] == out_len(consumed, 0, n, o, width, True), (rates, L, kind)
            got = np.concatenate(outs + [tail], 1)
            assert got.shape == ref.shape == (2, math.ceil(n * L / o)), (rates, L, kind, got.shape, ref.shape)
            assert sum(out_len(a, c, n, o, width) for a, c in zip(np.cumsum([0] + sizes[:-1]), sizes)) + tail.shape[1] == ref.shape[1]
            if got.size:
                assert np.abs(got - ref).max() < 1e-12, (rates, L, kind)


def test_output_length_helper_edges():
    out_len = _helper()
    n, o, width = 3, 2, 7                       # 16 -> 24 kHz
    assert out_len(0, width + o - 1, n, o, width) == 0 and out_len(0, width + o, n, o, width) == n
    assert out_len(0, 0, n, o, width) == 0 and out_len(0, 0, n, o, width, True) == 0
    assert out_len(0, 1, n, o, width, True) == 2                   # ceil(3 / 2)
    assert out_len(width + o, 0, n, o, width, True) == math.ceil(n * (width + o) / o) - n
    assert out_len(1 << 40, 2, n, o, width) == 3                   # 64-bit counts
    for bad in ((-1, 1, n, o, width), (0, -1, n, o, width), (0, 1, 0, o, width), (0, 1, n, 0, width), (0, 1, n, o, -1)):
        with pytest.raises(ValueError):
            out_len(*bad)


def test_latency_is_half_a_millisecond_at_16_and_24_khz():
    for orig, new in ((16000, 24000), (24000, 16000)):
        _, n, o, width = R.kernel(orig, new)
        assert (width + o - 1) / orig == pytest.approx(0.5e-3)


def test_no_cpu_fallback():
    from audiocodecs_amd import Encodec, Mimi, ResampleStream, _native, checkpoint
    from audiocodecs_amd.config import MIMI_TINY, TINY

    with pytest.raises(_native.NativeError, match="MI355X"):
        ResampleStream(16000, 24000, 2, device="cpu")
    for bad in ((0, 24000, 2), (16000, -1, 2), (16000.0, 24000, 2), (16000, 24000, 0), (16000, 24000, True), (16000, 24000, "2")):
        with pytest.raises(ValueError):
            ResampleStream(*bad, device="cpu")
    same = ResampleStream(24000, 24000, 2, device="cpu")          # equal rates: the input itself, as the one-shot returns it
    x = torch.zeros(2, 5)
    assert same.push(x) is x and same.finish().shape == (2, 0) and same.latency_samples == 0
    assert same.consumed == same.emitted == 5
    with pytest.raises(ValueError, match="finish"):
        same.push(x)
    same.reset()
    assert same.push(x) is x
    codecs = [Encodec(16000, state_dict=checkpoint.synthetic_state_dict(TINY, seed=0), config=TINY),
              Mimi(16000, state_dict=checkpoint.synthetic_mimi_state_dict(MIMI_TINY, seed=0), config=MIMI_TINY)]
    for codec in codecs:
        for fn in (codec.encode_stream, codec.decode_stream):
            with pytest.raises(ValueError, match="resampling"):     # the default keyword: as before
                fn(2, "cpu")
            with pytest.raises(_native.NativeError):               # resample=True: as the streams at the codec's own rate, no GPU no stream
                fn(2, "cpu", resample=True)
            with pytest.raises(ValueError):
                fn(0, "cpu", resample=True)
            with pytest.raises(TypeError):
                fn(2, "cpu", True)                                  # keyword-only
