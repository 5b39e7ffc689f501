"""Every sub-layer of the STREAMED Mimi transformer on its own against fp64.

`Mimi.encode_stream` / `decode_stream` and the session pools run a transformer of their own (csrc/mimi_stream.hip): RoPE at each
stream's absolute position (mstream_rope_kernel), online softmax over [ring || this push's keys] with the ring slot position % R
(mstream_attn_kernel), the append behind the attention (mstream_append_kernel), the up-sampler on [previous row | push]
(mstream_upsample_kernel) and, for pushes of few rows, mstream_linear_kernel.  With `ac_debug_capture` armed a push emits its
transformer's input and per layer `qkv` (rotated), `att` and the layer's output (include/audiocodecs_amd.h).  As in
tests/test_layer_isolation_gpu.py the GPU's OWN earlier taps are the inputs of the reference, so nothing upstream spends the budget:

    qkv   from the previous tap of the push (the transformer's input, or the previous layer's output)
    att   from this push's qkv tap and the k / v columns of the SAME STREAM's qkv taps of earlier pushes since its reset
    out   from the layer's input tap and its att tap
    up    (decode) from the qf taps: this push's rows and the previous push's last row

each by one function of tests/mimi_stream_layer_ref.py in fp64 (ref64) and fp32 (ref32), under that file's `_judge` and its bar,
|got - ref64| <= 5e-6 * max(1, max|ref64|) + 2e-5 * |ref64|, unchanged.  tests/test_mimi_stream_layers_cpu.py proves the
reference equal to the one-shot oracle layer, shows ref32 at most 0.1 of the bar on these cases and shows that a window of 249 or
251, a ring slot read one off, a missing append, the neighbour's ring or a position one off put every affected row more than 10
times (measured: 145 times and up) past it.  Only the bar and finiteness are asserted; e_gpu, e_ref, their ratio and the worst
|err| / tol go to the parity record (`mimi_stream_layers/...`) per tap and push, and as one row per kernel.

A failure names the push, the layer, the stream, the absolute position of the worst row, and the worst |err| / tol at positions 0,
249, 250, 251 and at the first and last row of the push.  The cases are listed in tests/mimi_stream_layer_cases.py."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mimi_stream_layer_cases as MC
import mimi_stream_layer_ref as R
import parity_record
from oracle import mimi_oracle as O
from test_gpu_parity import capture
from test_layer_isolation_gpu import _judge

pytestmark = pytest.mark.gpu

_CACHE = {}
CAP_FLOATS = 1 << 23          # one push: at most 260 rows x (512 + 8 x 2560) floats


def _weights(cfg_name, request):
    if ("W", cfg_name) not in _CACHE:
        cfg, sd = request.getfixturevalue("mimi_checkpoints")(cfg_name, 0)
        _CACHE["W", cfg_name] = (cfg, sd, O.cast_weights(sd), O.cast_weights(sd, torch.float64))
    return _CACHE["W", cfg_name]


def _codec(cfg_name, precision, request):
    if ("codec", cfg_name, precision) not in _CACHE:
        from audiocodecs_amd import Mimi

        cfg, sd, _, _ = _weights(cfg_name, request)
        c = Mimi(24000, num_codebooks=8, state_dict=sd, config=cfg, precision=precision).eval()
        c._native_for(torch.empty(0, device="cuda"))          # creates the native handle
        _CACHE["codec", cfg_name, precision] = c
    return _CACHE["codec", cfg_name, precision]


def _set_route(codec, value):
    from audiocodecs_amd._native import debug_set

    debug_set(codec, "mstream_skinny", value)


def _inputs(cfg_name, name, B, frames, direction, request):
    """The case's signal [B, frames * HOP] (encode) or the fp32 oracle's tokens of it [B, frames, K] (decode), on the GPU."""
    cfg, _, W, _ = _weights(cfg_name, request)
    sig = MC.signal(MC.SEED[name], B, frames)
    if direction == "encode":
        return sig.cuda()
    return MC.oracle_run((cfg_name, MC.SEED[name], B, frames), cfg, W, sig)["toks"].cuda()


def _cut(x, first, frames, direction):
    unit = MC.HOP if direction == "encode" else 1
    return x[:, first * unit:(first + frames) * unit].contiguous()


class Ledger:
    """What the test holds of every stream since its reset: the position, per layer the k / v columns of the GPU's own qkv taps (by
    absolute position), the last dequantised row.  It judges one captured push at a time and collects figures and failures."""

    def __init__(self, cfg_name, direction, case, request):
        self.cfg, _, self.W, self.W64 = _weights(cfg_name, request)
        self.direction, self.case, self.part = direction, case, MC.PARTS[direction]
        self.streams, self.figures, self.failures, self.taps = {}, {}, [], []
        self.npush = 0

    def reset(self, sid):
        c = self.cfg
        A = c.num_attention_heads * c.head_dim
        self.streams[sid] = {"pos": 0, "qf": None, "k": [torch.zeros(0, A) for _ in range(c.num_hidden_layers)],
                             "v": [torch.zeros(0, A) for _ in range(c.num_hidden_layers)]}

    def parse(self, flat, n, F):
        """The capture of one push of n rows and F frames -> {"qf", "x", "layers": [{"qkv", "att", "out"}]}, [n,T,*] each."""
        c = self.cfg
        H, A, T = c.hidden_size, c.num_attention_heads * c.head_dim, F * c.resample_stride
        shapes = ([("qf", (n, F, H))] if self.direction == "decode" else []) + [("x", (n, T, H))]
        for l in range(c.num_hidden_layers):
            shapes += [((l, "qkv"), (n, T, 3 * A)), ((l, "att"), (n, T, A)), ((l, "out"), (n, T, H))]
        need = sum(int(np.prod(s)) for _, s in shapes)
        assert flat.size == need, f"{self.case} push {self.npush}: {flat.size} captured floats, the tap list has {need}"
        out, off = {"layers": [{} for _ in range(c.num_hidden_layers)]}, 0
        for key, shape in shapes:
            t = torch.from_numpy(flat[off:off + int(np.prod(shape))]).view(shape)
            off += t.numel()
            if isinstance(key, tuple):
                out["layers"][key[0]][key[1]] = t
            else:
                out[key] = t
        return out

    def _one(self, name, got, ref64, ref32, sids, pos0):
        before = len(self.failures)
        _judge(SimpleNamespace(name=name, result=False), self.direction, self.case, got, ref64, ref32, self.figures, self.failures)
        if len(self.failures) > before:
            over = (got.double() - ref64).abs() / MC.bar(ref64)                 # [rows, T, C]
            over = torch.where(torch.isfinite(over), over, torch.full_like(over, float("inf")))
            b, t, _ = (int(v) for v in np.unravel_index(int(over.flatten().argmax()), over.shape))
            T = over.shape[1]
            named = {f"position {p}": p - pos0 for p in MC.NAMED_POSITIONS if pos0 <= p < pos0 + T}
            named.update({"first row": 0, "last row": T - 1})
            self.failures[-1] += (f"; push {self.npush}, streams {sids} at position {pos0}: worst row is stream {sids[b]} row {t}"
                                  f" = absolute position {pos0 + t}; worst |err|/tol at "
                                  + ", ".join(f"{k}: {float(over[:, r].max()):.3f}" for k, r in named.items()))

    def judge(self, flat, sids, F, only=None):
        """One captured push whose row i is stream sids[i].  `only`: the streams to judge (the others' rows still enter the ledger)."""
        cfg, W, W64, part = self.cfg, self.W, self.W64, self.part
        A = cfg.num_attention_heads * cfg.head_dim
        cap = self.parse(flat, len(sids), F)
        self.taps.append(cap)
        groups = {}                                             # position -> rows: streams at one position are judged as one tensor
        for i, s in enumerate(sids):
            if only is None or s in only:
                groups.setdefault(self.streams[s]["pos"], []).append(i)
        with torch.no_grad():
            for pos0, rows in groups.items():
                who = [sids[i] for i in rows]
                tag = f"push{self.npush}" + (f"/s{'+'.join(map(str, who))}" if len(groups) > 1 or only is not None else "")
                if self.direction == "decode":
                    qf = cap["qf"][rows]
                    prev = torch.stack([self.streams[s]["qf"] if self.streams[s]["qf"] is not None else torch.zeros(cfg.hidden_size) for s in who])
                    self._one(f"{tag}/up", cap["x"][rows], R.upsample(cfg, W64, prev.double(), qf.double()), R.upsample(cfg, W, prev, qf), who, pos0)
                x = cap["x"][rows]
                for l, t in enumerate(cap["layers"]):
                    qkv, att, out = t["qkv"][rows], t["att"][rows], t["out"][rows]
                    self._one(f"{tag}/L{l}/qkv", qkv, R.qkv_rot(cfg, W64, l, part, x.double(), pos0), R.qkv_rot(cfg, W, l, part, x, pos0), who, pos0)
                    q, k, v = qkv[..., :A], qkv[..., A:2 * A], qkv[..., 2 * A:]
                    kh = torch.stack([self.streams[s]["k"][l] for s in who])
                    vh = torch.stack([self.streams[s]["v"][l] for s in who])
                    self._one(f"{tag}/L{l}/att", att, R.attend(cfg, q.double(), kh.double(), vh.double(), k.double(), v.double(), pos0),
                              R.attend(cfg, q, kh, vh, k, v, pos0), who, pos0)
                    self._one(f"{tag}/L{l}/out", out, R.layer_out(cfg, W64, l, part, x.double(), att.double()), R.layer_out(cfg, W, l, part, x, att), who, pos0)
                    x = out
        for i, s in enumerate(sids):                            # the push enters every listed stream's history
            st = self.streams[s]
            for l, t in enumerate(cap["layers"]):
                st["k"][l] = torch.cat([st["k"][l], t["qkv"][i, :, A:2 * A]], 0)
                st["v"][l] = torch.cat([st["v"][l], t["qkv"][i, :, 2 * A:]], 0)
            st["pos"] += F * cfg.resample_stride
            if self.direction == "decode":
                st["qf"] = cap["qf"][i, -1]
        self.npush += 1

    def finish(self):
        """Record the figures per tap and push and one row per kernel; fail with every message."""
        kinds = {"up": "mstream_upsample_kernel", "qkv": "LN1 + qkv linear + mstream_rope_kernel", "att": "mstream_attn_kernel (+ mstream_append_kernel)",
                 "out": "o-proj + LN2 + MLP linears"}
        per_kernel = {}
        for kind, kernel in kinds.items():
            rows = [f for name, f in self.figures.items() if name.endswith("/" + kind)]
            if rows:
                per_kernel[kind] = {"kernel": kernel, "taps": len(rows), "e_gpu": max(r["e_gpu"] for r in rows), "e_ref": max(r["e_ref"] for r in rows),
                                    "ratio": max(r["ratio"] for r in rows), "worst_err_over_tol": max(r["worst_err_over_tol"] for r in rows)}
                print(f"{self.case} {self.direction} {kind:>4} over {len(rows)} taps: " + "  ".join(
                    f"{k} {v:.3e}" if k.startswith("e_") else f"{k} {v:.3f}" for k, v in per_kernel[kind].items() if k not in ("kernel", "taps")))
        parity_record.record("mimi_stream_layers", f"{self.case}/{self.direction}", per_tap=self.figures, per_kernel=per_kernel)
        assert self.npush > 0 and self.figures
        assert not self.failures, "\n".join(self.failures)


def _captured_push(codec, push):
    """push() under the hook -> (its result, the capture)."""
    return capture(codec, push, CAP_FLOATS)


# ---- lockstep streams ------------------------------------------------------------------------------------------------------------------
def _lockstep(cfg_name, name, B, schedule, direction, precision, route, variant, request):
    cfg, _, _, _ = _weights(cfg_name, request)
    codec = _codec(cfg_name, precision, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    x = _inputs(cfg_name, name, B, sum(schedule), direction, request)
    _set_route(codec, route)
    try:
        make = codec.encode_stream if direction == "encode" else codec.decode_stream
        hooked, plain = make(B), make(B)
        led = Ledger(cfg_name, direction, f"{cfg_name}_lockstep/{variant}", request)
        for b in range(B):
            led.reset(b)
        first = 0
        for f in schedule:
            piece = _cut(x, first, f, direction)
            got, flat = _captured_push(codec, lambda: hooked.push(piece))
            want = plain.push(piece)
            assert got.shape == want.shape and torch.equal(got, want), f"push at frame {first}: the hook changed the push's result"
            assert direction == "encode" or bool(torch.isfinite(got).all())
            led.judge(flat, list(range(B)), f)
            first += f
    finally:
        _set_route(codec, -1)
    return led


@pytest.mark.parametrize("precision", [None, "fp32_exact"], ids=["split16", "fp32_exact"])
def test_full_encode_stream_sub_layers_against_fp64(precision, request):
    """Full config, B = 1, pushes of 2, 4, 6, 116, 122, 260, 2, 248, 2, 10 rows (mimi_stream_layer_cases.FULL_FRAMES)."""
    cfg, _, _, _ = _weights("full", request)
    assert cfg.sliding_window == 250 and MC.starts_of(MC.FULL_FRAMES)[5] == 250 and MC.rows_of(MC.FULL_FRAMES)[5] > cfg.sliding_window - 1
    _lockstep("full", "full", 1, MC.FULL_FRAMES, "encode", precision, -1, precision or "split16", request).finish()


@pytest.mark.parametrize("route", [0, 1], ids=["tap_gemm", "skinny"])
def test_full_decode_stream_sub_layers_against_fp64(route, request):
    """The same schedule on the decode side, from the fp32 oracle's tokens of the same signal, the linear layers forced through the
    tap-GEMM (0) and through mstream_linear_kernel (1)."""
    _lockstep("full", "full", 1, MC.FULL_FRAMES, "decode", None, route, f"route{route}", request).finish()


@pytest.mark.parametrize("direction", ["encode", "decode"])
def test_tiny_stream_sub_layers_against_fp64(direction, request):
    """Window 6, ring 5, head_dim 16, 4 heads, B = 3, pushes of 2, 2, 4, 6, 2, 8 rows: almost every push has T >= R."""
    _lockstep("tiny", "tiny", 3, MC.TINY_FRAMES, direction, None, -1, "auto", request).finish()


# ---- session pools ---------------------------------------------------------------------------------------------------------------------
def _pool_push(codec, pool, plain, slots, piece, led, F):
    """One slot push under the hook on `pool`, the same push without it on `plain`: the same bits, and the capture is judged."""
    res, flat = _captured_push(codec, lambda: pool.push(slots, piece))
    want = plain.push(slots, piece)
    for g, w in zip(res, want):
        assert g.shape == w.shape and torch.equal(g, w), "the hook changed the push's result"
    led.judge(flat, slots, F)


def _open_slot(pool, slot):
    """Open exactly `slot`: `open` hands out the lowest free one."""
    taken = []
    while True:
        s = pool.open()
        if s == slot:
            break
        taken.append(s)
    for s in taken:
        pool.close(s)


@pytest.mark.parametrize("direction", ["encode", "decode"])
def test_slot_push_sub_layers_against_fp64(direction, request):
    """Full config, capacity 3.  Slot 0 runs alone to position 300 (past a wrapped ring), slot 2 opens, one push of 3 frames lists
    [2, 0] -- a row at position 0 and a row past the wrap, in a non-identity order -- and the next lists [0, 2].  Every push is
    captured (the history is needed); in the joint pushes each row is judged against its own stream's history."""
    codec = _codec("full", None, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    alone, joint = MC.SLOT_ALONE_FRAMES, MC.SLOT_JOINT
    x0 = _inputs("full", "slot0", 1, sum(alone) + sum(f for _, f in joint), direction, request)
    x2 = _inputs("full", "slot2", 1, sum(f for _, f in joint), direction, request)
    make = codec.encode_sessions if direction == "encode" else codec.decode_sessions
    pool, plain = make(3), make(3)
    led = Ledger("full", direction, "full_slots", request)
    for p in (pool, plain):
        _open_slot(p, 0)
    led.reset(0)
    at = {0: 0, 2: 0}
    for f in alone:
        _pool_push(codec, pool, plain, [0], _cut(x0, at[0], f, direction), led, f)
        at[0] += f
    assert led.streams[0]["pos"] == 300 > codec.config.sliding_window
    for p in (pool, plain):
        _open_slot(p, 2)
        assert p.active == [0, 2]
    led.reset(2)
    for slots, f in joint:
        piece = torch.cat([_cut({0: x0, 2: x2}[s], at[s], f, direction) for s in slots], 0)
        _pool_push(codec, pool, plain, slots, piece, led, f)
        for s in slots:
            at[s] += f
    assert led.streams[2]["pos"] == 10 and led.streams[0]["pos"] == 310
    led.finish()


@pytest.mark.parametrize("direction", ["encode", "decode"])
def test_a_reopened_slot_reads_nothing_of_the_stale_ring(direction, request):
    """Tiny config, capacity 2 (a reset does not touch the rings).  Slot 1 runs 8 rows past its ring of 5 -- NaN samples on the
    encode side, ordinary tokens on the decode side, where NaN cannot enter -- is closed and reopened (a slot reset) and then fed a
    clean input: its taps are finite and meet the bar with an EMPTY history.  The whole sequence runs a second time with another
    (clean) first session in slot 1: slot 0's taps of every push, and the reopened slot's taps, are the same bits in both runs."""
    codec = _codec("tiny", None, request)
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    first, second = MC.STALE_FIRST_FRAMES, MC.STALE_SECOND_FRAMES
    x0 = _inputs("tiny", "stale0", 1, sum(first) + sum(second), direction, request)
    x1 = _inputs("tiny", "stale1", 1, sum(second), direction, request)
    other = _inputs("tiny", "tiny", 1, sum(first), direction, request)               # the first session of slot 1 in the second run
    spoiled = torch.full_like(other, float("nan")) if direction == "encode" else _inputs("tiny", "slot2", 1, sum(first), direction, request)
    make = codec.encode_sessions if direction == "encode" else codec.decode_sessions
    runs = []
    for r, before in enumerate((spoiled, other)):
        pool = make(2)
        led = Ledger("tiny", direction, f"tiny_stale_ring/run{r}", request)
        assert [pool.open(), pool.open()] == [0, 1]
        led.reset(0), led.reset(1)
        at = 0
        for f in first:
            piece = torch.cat([_cut(x0, at, f, direction), _cut(before, at, f, direction)], 0)
            _, flat = _captured_push(codec, lambda: pool.push([0, 1], piece))
            led.judge(flat, [0, 1], f, only=[0] if r == 0 and direction == "encode" else None)      # (slot 1's rows are NaN there)
            at += f
        assert led.streams[1]["pos"] == 8 > codec.config.sliding_window - 1
        if r == 0 and direction == "encode":
            assert all(bool(torch.isnan(t["att"][1]).all()) for cap in led.taps for t in cap["layers"]), "slot 1's ring was to hold NaN"
        pool.close(1)
        assert pool.open() == 1
        led.reset(1)
        for i, f in enumerate(second):
            piece = torch.cat([_cut(x0, at, f, direction), _cut(x1, at - sum(first), f, direction)], 0)
            res, flat = _captured_push(codec, lambda: pool.push([0, 1], piece))
            assert all(bool(torch.isfinite(t.float()).all()) for t in res)
            led.judge(flat, [0, 1], f)
            assert all(bool(torch.isfinite(t[k]).all()) for t in led.taps[-1]["layers"] for k in t), f"push {i} after the reopening: a tap is not finite"
            at += f
        runs.append(led)
    a, b = runs
    for i, (ca, cb) in enumerate(zip(a.taps, b.taps)):
        rows = [0] if i < len(first) else [0, 1]
        for l, (ta, tb) in enumerate(zip(ca["layers"], cb["layers"])):
            for k in ta:
                assert torch.equal(ta[k][rows], tb[k][rows]), f"push {i} layer {l} {k}: rows {rows} depend on what slot 1 held before"
    for led in runs:
        led.finish()


# ---- which kernels ran -------------------------------------------------------------------------------------------------------------------
def test_stream_kernels_run_under_the_hook(request):
    """The tests above judge the kernels that run WITH the hook armed; the hook only adds copies, and this pins the names (split16,
    a push of 3 frames behind a push of 1, lockstep and as a slot push): mstream_rope / attn / append always, mstream_upsample on decode,
    mstream_linear_kernel only with the route forced to 1, and a row-mode tap-GEMM launch of the qkv projection ([rows, 512] x
    [512, 1536]) on encode and with the route forced to 0, on the full config; the stream kernels on the tiny config as well."""
    from audiocodecs_amd._native import debug_set

    cfg, _, _, _ = _weights("full", request)
    A, H = cfg.num_attention_heads * cfg.head_dim, cfg.hidden_size

    def names(direction, route, pool, cfg_name="full"):
        codec = _codec(cfg_name, None, request)
        x = _inputs(cfg_name, "full", 1, 4, direction, request)
        _set_route(codec, route)
        debug_set(codec, "prof_detail", 1)
        try:
            if pool:
                s = codec.encode_sessions(2) if direction == "encode" else codec.decode_sessions(2)
                assert [s.open(), s.open()] == [0, 1]
                s.push([1], _cut(x, 0, 1, direction))
                push = lambda: s.push([1], _cut(x, 1, 3, direction))          # noqa: E731
            else:
                s = codec.encode_stream(1) if direction == "encode" else codec.decode_stream(1)
                s.push(_cut(x, 0, 1, direction))
                push = lambda: s.push(_cut(x, 1, 3, direction))                # noqa: E731
            stats = codec.profile_kernels(lambda: _captured_push(codec, push))
        finally:
            debug_set(codec, "prof_detail", 0)
            _set_route(codec, -1)
        got = {s[0] for s in stats}
        print(cfg_name, direction, route, "pool" if pool else "lockstep", sorted(got))
        return got

    qkv_gemm = rf"tap_gemm\w*_kernel<.*> B1 M6 N{3 * A} K{H} J1 s1$"
    for pool in (False, True):
        enc = names("encode", -1, pool)
        assert {"mstream_rope_kernel", "mstream_attn_kernel", "mstream_append_kernel"} <= enc, enc
        assert "mstream_linear_kernel" not in enc and "mstream_upsample_kernel" not in enc, enc
        assert any(re.match(qkv_gemm, n) for n in enc), enc
        for route in (0, 1):
            dec = names("decode", route, pool)
            assert {"mstream_rope_kernel", "mstream_attn_kernel", "mstream_append_kernel", "mstream_upsample_kernel"} <= dec, dec
            assert ("mstream_linear_kernel" in dec) == (route == 1), dec
            assert any(re.match(qkv_gemm, n) for n in dec) == (route == 0), dec
        assert not any(n.startswith("attention") for n in enc | dec), enc | dec
        # the tiny config (head_dim 16): the same stream kernels; its linear routes are not pinned
        enc, dec = names("encode", -1, pool, "tiny"), names("decode", -1, pool, "tiny")
        assert {"mstream_rope_kernel", "mstream_attn_kernel", "mstream_append_kernel"} <= enc and "mstream_upsample_kernel" not in enc, enc
        assert {"mstream_rope_kernel", "mstream_attn_kernel", "mstream_append_kernel", "mstream_upsample_kernel"} <= dec, dec
        assert not any(n.startswith("attention") for n in enc | dec), enc | dec
