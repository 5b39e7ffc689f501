"""The per-slot resampler and the resampling session pools off the GPU (audiocodecs_amd.ResampleSlots, sessions.py
`SessionPool(..., resample=True)`).

`ResampleSlots` keeps its host side (per-slot counts, the output length of a push, who is closed) apart from the three methods that
touch the device state.  `ToySlots` replaces those three with the chunked fp64 restatement of tests/test_resample_stream.py, one
`NumpyStream` per slot, which knows nothing of the output-length rule: every push is checked against what the restatement emits for
that slot.  The pool runs on the toy backend of tests/test_stream_host.py with `ToySlots` at its boundary; every session is shadowed by
a restatement of its own (a lone `NumpyStream`, the per-row hold rule, the toy codec) fed the same pieces, so its results are compared
exactly.  The GPU side is tests/test_resample_slots_gpu.py."""
import math
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import resample_oracle as R
from test_resample_stream import RATES, NumpyStream, _helper
from test_stream_host import FLAVOURS, HOP, K, ToyBackend, ToyEncodeSessions, toy_codec

from audiocodecs_amd.resample import ResampleSlots
from audiocodecs_amd.sessions import SessionPool, plan_push

CAP = 5


class ToySlots(ResampleSlots):
    """ResampleSlots on CPU tensors: the host side is the real one, the state is one chunked fp64 restatement per slot."""

    def _attach(self, kern, device):
        self.device = torch.device("cpu")
        self._np = [NumpyStream(self.orig_freq, self.new_freq, 1) for _ in range(self.capacity)]     # the whole reset
        self.restarts, self.lens = [], None

    def _restart_rows(self, slots):
        assert len(set(slots)) == len(slots) and all(type(s) is int and 0 <= s < self.capacity for s in slots)
        for s in slots:
            self._np[s] = NumpyStream(self.orig_freq, self.new_freq, 1)
        self.restarts.append(list(slots))

    def _push_rows(self, slots, counts, x, L, m, finish):
        assert len(set(slots)) == len(slots) and tuple(x.shape) == (len(slots), L) and (L or finish)
        y = torch.full((len(slots), m), float("nan"))
        self.lens = []
        for i, s in enumerate(slots):
            st = self._np[s]
            assert st is not None and st.total == counts[i], f"slot {s}: the caller's count {counts[i]} is not the state's {st.total}"
            out = st.push(x[i:i + 1].numpy())
            if finish:
                out = np.concatenate([out, st.finish()], 1)
                self._np[s] = None                                   # closed: only a restart brings it back
            assert out.shape[1] <= m
            y[i, :out.shape[1]] = torch.from_numpy(out[0].astype(np.float32))
            self.lens.append(out.shape[1])
        return y


def pieces_for(o):
    return [0, 1, 2, 7, o - 1, o, o + 1, 213, 320, 1001]


# ---- 1. the resampler's host side ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_out_len_per_slot_against_the_chunked_restatement(rates):
    _helper()
    rng = random.Random(f"slots/{rates}")
    nprng = np.random.default_rng(5)
    rs = ToySlots(*rates, CAP)
    n, o = rs.n, rs.o
    assert rs.taps == 2 * rs.width + o and rs.latency_samples == rs.width + o - 1
    sig = {s: np.zeros((1, 0)) for s in range(CAP)}          # what every slot has been fed since its restart
    got = {s: [] for s in range(CAP)}
    live, phases_differ, lens_differ, finished = [], 0, 0, 0
    for step in range(200):
        if step % 9 == 0 and len(live) < CAP:                # slots start at different times: their counts differ mod o
            s = min(set(range(CAP)) - set(live))
            rs.restart([s])
            assert rs.consumed[s] == rs.emitted[s] == 0
            sig[s], got[s] = np.zeros((1, 0)), []
            live.append(s)
        if not live:
            continue
        slots = rng.sample(live, rng.randint(1, len(live)))
        L = rng.choice(pieces_for(o))
        fin = rng.random() < 0.08
        x = nprng.standard_normal((len(slots), L))
        want = [rs.out_len(s, L, fin) for s in slots]
        before = [(rs.consumed[s], rs.emitted[s]) for s in slots]
        phases_differ += len({rs.consumed[s] % o for s in slots}) > 1
        out = rs.push(slots, torch.from_numpy(x.astype(np.float32)), finish=fin)
        if L or fin:
            assert rs.lens == want, (rates, step, slots, L, fin)      # the restatement emitted what the rule says, slot by slot
        lens_differ += len(set(want)) > 1
        for i, s in enumerate(slots):
            assert out[i].shape == (want[i],) and out[i].dtype == torch.float32 and not bool(torch.isnan(out[i]).any())
            assert (rs.consumed[s], rs.emitted[s]) == (before[i][0] + L, before[i][1] + want[i])
            assert fin or want[i] % n == 0
            sig[s] = np.concatenate([sig[s], x[i:i + 1].astype(np.float32).astype(np.float64)], 1)
            got[s].append(out[i].numpy())
            if fin:
                total = sig[s].shape[1]
                assert rs.emitted[s] == math.ceil(n * total / o)
                whole = np.concatenate(got[s])
                if total:
                    assert np.abs(whole - R.resample(sig[s], *rates)[0]).max() < 1e-6
                with pytest.raises(ValueError, match="finish"):
                    rs.push([s], torch.zeros(1, 3))
                with pytest.raises(ValueError, match="finish"):
                    rs.push([s], torch.zeros(1, 0), finish=True)
                live.remove(s)
                finished += 1
    assert finished >= 5 and phases_differ >= 10 and lens_differ >= 10
    for s in list(live):                                     # whoever is still open closes now: the same total
        tail = rs.push([s], torch.zeros(1, 0), finish=True)[0]
        assert tail.shape[0] == rs.emitted[s] - sum(len(g) for g in got[s])
        assert rs.emitted[s] == math.ceil(n * sig[s].shape[1] / o)


def test_slots_argument_checks_and_equal_rates():
    from audiocodecs_amd import _native

    _helper()
    with pytest.raises(_native.NativeError, match="MI355X"):
        ResampleSlots(16000, 24000, 2, device="cpu")
    for bad in ((0, 24000, 2), (16000, -1, 2), (16000.0, 24000, 2), (16000, 24000, 0), (16000, 24000, True), (16000, 24000, "2")):
        with pytest.raises(ValueError):
            ResampleSlots(*bad, device="cpu")
    rs = ToySlots(16000, 24000, 3)
    x = torch.zeros(2, 5)
    for bad in ([0, 3], [-1, 0], [True, 0], [0.0, 1], 1):
        with pytest.raises(ValueError, match="slots"):
            rs.push(bad, x)
    with pytest.raises(ValueError, match="twice"):
        rs.push([1, 1], x)
    with pytest.raises(ValueError, match="twice"):
        rs.restart([2, 2])
    for wrong in (x[:1], x[0], x.double(), x[:, None]):
        with pytest.raises(ValueError, match="expects"):
            rs.push([0, 1], wrong)
    with pytest.raises(ValueError):
        rs.out_len(3, 5)
    assert rs.consumed == [0, 0, 0] and rs.restarts == [] and rs.lens is None        # the refusals reached nothing
    same = ResampleSlots(24000, 24000, 3, device="cpu")      # equal rates: the input itself
    out = same.push([2, 0], x)
    assert torch.equal(out[0], x[0]) and same.consumed == [5, 0, 5] and same.emitted == [5, 0, 5] and same.latency_samples == 0
    assert same.out_len(1, 9) == 9 and same.push([1], x[:1], finish=True)[0].shape == (5,)
    with pytest.raises(ValueError, match="finish"):
        same.push([1], x[:1])
    same.restart([1])
    assert same.consumed[1] == 0 and same.push([1], x[:1])[0].shape == (5,)


# ---- 2. the pool with a resampler at its boundary ------------------------------------------------------------------------------------
CODEC16 = SimpleNamespace(sample_rate=16000, config=SimpleNamespace(sampling_rate=24000))
CODEC24 = SimpleNamespace(sample_rate=24000, config=SimpleNamespace(sampling_rate=24000))


class _OnToy16:
    def __init__(self, flavour, n, resample, codec=CODEC16):
        f = FLAVOURS[flavour]
        super().__init__(codec, ToyBackend(self._kind, f["warmup"], f["together"]), n, K, resample)


class ToyEncodePool(_OnToy16, SessionPool):
    _kind = "encode"
    _resampler = ToySlots


class ToyDecodePool(_OnToy16, SessionPool):
    _kind = "decode"
    _resampler = ToySlots


class Shadow:
    """One session restated: a lone resampler, the per-row hold rule and the toy codec, fed the same pieces."""

    def __init__(self, kind, warmup):
        self.kind, self.warmup = kind, warmup
        self.rs = NumpyStream(16000, 24000, 1) if kind == "encode" else NumpyStream(24000, 16000, 1)
        self.held = torch.empty(0) if kind == "encode" else torch.empty(0, K, dtype=torch.int64)
        self.ran = self.chk = 0
        self.emitted = 0          # resampler outputs so far

    def _resample(self, x, finish):
        out = self.rs.push(x.view(1, -1).numpy()) if not finish else np.concatenate([self.rs.push(np.zeros((1, 0))), self.rs.finish()], 1)
        self.emitted += out.shape[1]
        return torch.from_numpy(out[0].astype(np.float32))

    def _frames(self):
        unit = HOP if self.kind == "encode" else 1
        F = self.held.shape[0] // unit
        F = 0 if (self.ran == 0 and F < self.warmup) else F
        run, self.held = self.held[:F * unit], self.held[F * unit:]
        out, self.ran, self.chk = toy_codec(self.kind, run, self.ran, self.chk)
        return F, out

    def push(self, x, finish=False):
        """Returns (frames run, incoming units at the codec's rate, the result)."""
        if self.kind == "encode":
            r = self._resample(x, finish)
            self.held = torch.cat([self.held, r])
            F, out = self._frames()
            return F, r.shape[0], out.view(-1, K)
        if finish:
            return 0, 0, self._resample(None, True)
        self.held = torch.cat([self.held, x])
        F, out = self._frames()
        return F, x.shape[0], (self._resample(out, False) if F else torch.empty(0))


def payload(rng, kind, rows, units):
    g = torch.Generator().manual_seed(rng.randrange(1 << 30))
    if kind == "encode":
        return torch.randint(-50, 50, (rows, units), generator=g).float()
    return torch.randint(0, 1000, (rows, units, K), generator=g)


@pytest.mark.parametrize("kind", ["encode", "decode"])
@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_resampling_pool_sessions_match_their_restatement(flavour, kind):
    _helper()
    rng = random.Random(f"rpool/{flavour}/{kind}")
    warmup, unit = FLAVOURS[flavour]["warmup"], HOP if kind == "encode" else 1
    pool = (ToyEncodePool if kind == "encode" else ToyDecodePool)(flavour, CAP, True)
    rs = pool._rs
    assert isinstance(rs, ToySlots) and (rs.orig_freq, rs.new_freq) == ((16000, 24000) if kind == "encode" else (24000, 16000))
    sizes = [0, 1, 2, 3, 5, 8, 13, 31, 2 * warmup * HOP] if kind == "encode" else [0, 1, 1, 2, 3, warmup, warmup + 2]
    shadow, opened, ragged, split, held_fresh, finished = {}, [0] * CAP, 0, 0, 0, 0
    for step in range(320):
        assert pool.active == sorted(shadow)
        r = rng.random()
        p_open, p_close = (0.4, 0.03) if (step // 25) % 2 == 0 else (0.05, 0.2)
        live = [s for s in sorted(shadow) if not shadow[s].done]
        if (r < p_open or not shadow) and len(shadow) < CAP:
            before = len(rs.restarts)
            slot = pool.open()
            assert slot == min(set(range(CAP)) - set(shadow)) and rs.restarts[before:] == [[slot]]       # `open` restarts the resampler slot
            assert rs.consumed[slot] == rs.emitted[slot] == 0 and pool.frames(slot) == 0 and pool.pending(slot) == 0
            shadow[slot] = Shadow(kind, warmup)
            shadow[slot].done = False
            opened[slot] += 1
        elif r < p_open + p_close and shadow:
            slot = rng.choice(sorted(shadow))
            pool.close(slot)
            del shadow[slot]
        elif r < p_open + p_close + 0.06 and live:
            slot = rng.choice(live)
            sh, calls = shadow[slot], len(pool._be.calls)
            F, _, want = sh.push(None, finish=True)
            got = pool.finish(slot)
            assert got.dtype == want.dtype and torch.equal(got, want), (step, slot)
            assert pool._be.calls[calls:] == ([(F, [slot])] if F else [])
            assert pool.frames(slot) == sh.ran and pool.pending(slot) == sh.held.shape[0]
            total = rs.consumed[slot]
            assert sh.emitted == rs.emitted[slot] == math.ceil(rs.n * total / rs.o)                         # the one-shot length
            for call in (lambda: pool.push([slot], payload(rng, kind, 1, 2)), lambda: pool.finish(slot)):
                with pytest.raises(ValueError, match="finish"):
                    call()
            sh.done = True
            finished += 1
        elif live:
            slots = rng.sample(live, rng.randint(1, len(live)))
            x = payload(rng, kind, len(slots), rng.choice(sizes))
            state = [(pool.pending(s), pool.frames(s)) for s in slots]
            calls = len(pool._be.calls)
            got = pool.push(slots, x)
            res = [shadow[s].push(x[i]) for i, s in enumerate(slots)]
            incoming = [m for _, m, _ in res]
            plan = plan_push([p for p, _ in state], [f for _, f in state], incoming, unit, warmup)
            assert pool._be.calls[calls:] == [(F, [slots[i] for i in rows]) for F, rows in plan]              # the right F groups
            ragged += len(set(incoming)) > 1
            split += len(plan) > 1
            for i, s in enumerate(slots):
                F, _, want = res[i]
                assert got[i].dtype == want.dtype and torch.equal(got[i], want), (step, s)
                assert pool.frames(s) == shadow[s].ran and pool.pending(s) == shadow[s].held.shape[0]
                assert rs.emitted[s] == shadow[s].emitted
                if state[i][1] == 0 and F == 0 and pool.pending(s) >= unit:
                    held_fresh += 1                               # whole frames wait: a fresh slot inside its warm-up
                    assert pool.pending(s) < warmup * unit and got[i].shape[0] == 0
    assert min(opened) >= 2 and finished >= 5
    if kind == "encode":
        assert ragged >= 20 and split >= 10                   # rows of one push brought different numbers of resampled samples
    if warmup > 1:
        assert held_fresh >= 5                                # ... counted in samples at the codec's rate


def test_resample_false_and_equal_rates_are_the_plain_pool():
    rng = random.Random("plain")
    plain = ToyEncodeSessions("encodec_like", CAP)
    pools = [ToyEncodePool("encodec_like", CAP, False), ToyEncodePool("encodec_like", CAP, True, CODEC24), plain]
    assert all(p._rs is None for p in pools)
    for p in pools:
        assert [p.open(), p.open(), p.open()] == [0, 1, 2]
    for _ in range(30):
        slots = rng.sample([0, 1, 2], rng.randint(1, 3))
        x = payload(rng, "encode", len(slots), rng.choice([0, 3, 4, 9, 30]))
        outs = [p.push(slots, x) for p in pools]
        for got in outs[:2]:
            assert all(torch.equal(a, b) for a, b in zip(got, outs[2]))
    assert plain.frames(0) > 7
    for p in pools[:2]:
        assert [p._be.calls, [p.pending(s) for s in range(3)]] == [plain._be.calls, [plain.pending(s) for s in range(3)]]
        assert p.finish(1).shape == (0, K)                    # nothing to flush without a resampler
        with pytest.raises(ValueError, match="finish"):
            p.push([1], torch.zeros(1, 4))
        assert p.push([0, 2], torch.zeros(2, 4))[0].shape == (1, K)     # the neighbours run on
        p.close(1)
        assert p.open() == 1 and p.push([1], torch.zeros(1, 4))[0].shape == (0, K)
    dec = ToyDecodePool("mimi_like", 2, False)
    assert dec.open() == 0 and dec.finish(0).shape == (0,)
