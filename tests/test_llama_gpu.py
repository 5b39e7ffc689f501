"""The Llama decoder on the GPU (audiocodecs_amd.llama) against tests/llama_ref.py.  The bound of a tensor is
K = 8 times the error of the fp32 statement against the fp64 statement on the same inputs, computed here, never from the library's output.
Cached steps are teacher-forced: the library's own history goes through the fp64 statement in one full forward, so that one flipped
near-tie cannot cascade."""
import ctypes as C

import numpy as np
import pytest
import torch

import llama_ref as R
import sampling_ref as S
from audiocodecs_amd import _native, prng
from audiocodecs_amd.llama import LlamaDecoder

pytestmark = pytest.mark.gpu

_DEC, _RUNS, _TEACHER = {}, {}, {}


def decoder(name):
    if name not in _DEC:
        _DEC[name] = LlamaDecoder(state_dict=R.weights(R.CONFIGS[name]), config=R.CONFIGS[name])
    return _DEC[name]


def run(name, B, P, steps, top_p, temp, eos_id=-1, seed=11, offset=7, use_graph=True):
    """One `generate(..., return_logits=True)` per distinct call: (rows, logits [n, B, C] on the CPU, bos, prompt)."""
    key = (name, B, P, steps, top_p, temp, eos_id, seed, offset, use_graph)
    if key not in _RUNS:
        cfg = R.CONFIGS[name]
        toks, prompt = R.inputs(cfg, B, P, 1)
        rows, log = decoder(name).generate(toks.cuda(), eos_id, prompt.cuda() if prompt is not None else None, max_gen_toks=steps, top_p=top_p, temp=temp,
                                           seed=seed, offset=offset, return_logits=True, use_graph=use_graph)
        _RUNS[key] = ([r.cpu() for r in rows], log.cpu(), toks, prompt)
    return _RUNS[key]


def teacher(name, rows, bos, prompt):
    """The statements' logits of every step on the history [prompt | bos | rows]: (fp64 [steps, B, C], the fp32 statement's error)."""
    key = (name, tuple(tuple(r.tolist()) for r in rows), None if prompt is None else prompt.shape[1])
    if key not in _TEACHER:
        cfg = R.CONFIGS[name]
        hyp = torch.stack(rows)
        P, n = 0 if prompt is None else prompt.shape[1], hyp.shape[1]
        out = []
        for dtype in (torch.float64, torch.float32):
            s = R.Statement(cfg, R.weights(cfg), dtype)
            embs = torch.cat([s.embed(bos, prompt), s.embed(hyp[:, :-1], curr_pos=1)], dim=1)
            out.append(s.forward(embs)[:, P:P + n].transpose(0, 1))
        _TEACHER[key] = (out[0], R.err(out[1], out[0]))
    return _TEACHER[key]


def check(name, got, s64, s32):
    bound = R.K_BOUND * R.err(s32, s64)
    e = R.err(got.cpu(), s64)
    print(f"  {name}: error {e:.3g}, bound {bound:.3g}")
    assert tuple(got.shape) == tuple(s64.shape), name
    assert bound > 0.0 and e <= bound, (name, e, bound)
    return bound


@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_prefill_stages(name, B):
    cfg = R.CONFIGS[name]
    dec = decoder(name)
    toks, prompt = R.inputs(cfg, B, 6, 21)
    embs = dec.embed(toks.cuda(), prompt.cuda() if prompt is not None else None)
    logits, state, st = dec.forward(embs, return_stages=True)
    T = embs.shape[1]
    assert state.pos == T and T == 21 + (6 if prompt is not None else 0)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        s = R.Statement(cfg, R.weights(cfg), dtype)
        stages = {}
        e = s.embed(toks, prompt)
        ref[dtype] = (e, s.forward(e, stages), stages)
    (e64, l64, g64), (e32, l32, g32) = ref[torch.float64], ref[torch.float32]
    if prompt is not None:
        check("embed", embs, e64, e32)
    else:
        assert torch.equal(embs.cpu().double(), e64)
    for l in range(cfg.n_layers):
        check(f"q[{l}]", st["q"][l], g64["q"][l], g32["q"][l])
        check(f"k[{l}]", state.kv(l, cfg.n_kv_heads, cfg.head_dim)[0][:, :T], g64["k"][l], g32["k"][l])
        check(f"attn[{l}]", st["attn"][l], g64["attn"][l], g32["attn"][l])
        check(f"layer_out[{l}]", st["layer_out"][l], g64["layer_out"][l], g32["layer_out"][l])
    check("final_norm", st["final_norm"], g64["final_norm"], g32["final_norm"])
    bound = check("logits", logits, l64, l32)
    assert torch.equal(state.logits(cfg.vocab_size), logits[:, -1])          # the pending row
    if name == "TINY_G2":
        w = R.Statement(cfg, R.weights(cfg), torch.float64, wrong_grouping=True)
        assert R.err(logits.cpu(), w.forward(w.embed(toks, prompt))) > bound


# B = 3, 5 and 9: the row counts at which the linear kernels take 2, 4 and 8 rows per pass (9: a second, partial pass)
@pytest.mark.parametrize("name,B,P,steps", [("TINY", 3, 6, 200), ("TINY", 3, 500, 80), ("TINY_HD128", 3, 6, 200), ("TINY", 5, 6, 40), ("TINY_HD128", 9, 6, 40)])
def test_cached_steps_teacher_forced(name, B, P, steps):
    rows, log, bos, prompt = run(name, B, P, steps, 0.9, 1.0)
    assert [len(r) for r in rows] == [steps] * B and log.shape == (steps, B, R.CONFIGS[name].vocab_size)
    s64, err32 = teacher(name, rows, bos, prompt)
    e = (log.double() - s64).abs().amax(dim=(1, 2))
    print(f"  {name} P={P}: worst step error {float(e.max()):.3g} at step {int(e.argmax())}, bound {R.K_BOUND * err32:.3g}")
    assert err32 > 0.0 and float(e.max()) <= R.K_BOUND * err32


@pytest.mark.parametrize("top_p,temp", [(0.9, 1.0), (0.5, 0.7)])
@pytest.mark.parametrize("name", ["TINY", "TINY_HD128"])
def test_sampling_exactness(name, top_p, temp):
    B, steps, seed, offset = 3, 200, 11, 7
    rows, log, _, _ = run(name, B, 6, steps, top_p, temp, seed=seed, offset=offset)
    got = torch.stack(rows).T.reshape(-1).numpy()                 # row r of step s is element offset + s B + r
    want = S.sample(log.reshape(steps * B, -1).numpy(), temp=temp, top_p=top_p, seed=seed, offset=offset)
    share = S.compare(got, *want)
    print(f"  {name} top_p={top_p} temp={temp}: {100 * share:.2f} % of {steps * B} draws excused")


@pytest.mark.parametrize("name", ["TINY", "TINY_HD128"])
def test_greedy_is_argmax(name):
    B, steps = 3, 200
    rows, log, bos, prompt = run(name, B, 6, steps, 0.0, 1.0)
    got = torch.stack(rows).T                                     # [steps, B]
    assert torch.equal(got, log.argmax(dim=-1))
    s64, err32 = teacher(name, rows, bos, prompt)
    sure = R.top2_gap(s64) > R.GAP_FACTOR * err32
    print(f"  {name}: {int((~sure).sum())} of {sure.numel()} steps within the gap")
    assert torch.equal(got[sure], s64.argmax(dim=-1)[sure]) and float((~sure).float().mean()) <= 0.03


def test_eos_lengths():
    name, B, steps = "TINY", 3, 60
    free, _, _, _ = run(name, B, 6, steps, 0.0, 1.0)
    assert [len(r) for r in free] == [steps] * B                  # eos_id = -1: every row returns max_gen_toks
    hyp = torch.stack(free)
    eos = next(int(t) for t in hyp[0, 5:] if any(int(t) not in r.tolist() for r in free[1:]))      # ends row 0, not every row
    want = R.lens_of(hyp, eos)
    assert want[0] < steps and max(want) == steps
    rows, log, _, _ = run(name, B, 6, steps, 0.0, 1.0, eos_id=eos)
    assert [len(r) for r in rows] == want
    for i in range(B):
        assert torch.equal(rows[i], hyp[i, :want[i]]) and eos not in rows[i].tolist()
    assert log.shape[0] == steps
    # one row: generation ends with it, polls and replays behind it change nothing
    one, _, _, _ = run(name, 1, 6, 200, 0.0, 1.0)
    eos1 = int(one[0][37])
    n = one[0].tolist().index(eos1)
    rows1, log1, _, _ = run(name, 1, 6, 200, 0.0, 1.0, eos_id=eos1)
    assert torch.equal(rows1[0], one[0][:n]) and log1.shape[0] == n + 1


def test_repeat_and_graph_are_bit_identical():
    a = run("TINY_HD128", 3, 6, 40, 0.9, 1.0)
    cfg = R.CONFIGS["TINY_HD128"]
    toks, prompt = a[2], a[3]
    rows, log = decoder("TINY_HD128").generate(toks.cuda(), -1, prompt.cuda(), max_gen_toks=40, top_p=0.9, temp=1.0, seed=11, offset=7, return_logits=True)
    assert all(torch.equal(x, y.cpu()) for x, y in zip(a[0], rows)) and torch.equal(a[1], log.cpu())
    b = run("TINY_HD128", 3, 6, 40, 0.9, 1.0, use_graph=False)
    assert all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and torch.equal(a[1], b[1])
    assert log.shape == (40, 3, cfg.vocab_size)


def test_forward_with_state_appends():
    cfg, dec = R.TINY, decoder("TINY")
    toks, prompt = R.inputs(cfg, 2, 6, 9)
    embs = dec.embed(toks.cuda(), prompt.cuda())
    T = embs.shape[1] - 1
    _, state = dec.forward(embs[:, :T], capacity=T + 1)
    assert state.pos == T
    last, state2 = dec.forward(embs[:, T:], state=state)
    assert state2 is state and state.pos == T + 1
    out = []
    for dtype in (torch.float64, torch.float32):
        s = R.Statement(cfg, R.weights(cfg), dtype)
        out.append(s.forward(s.embed(toks, prompt))[:, T:])
    check("the appended row", last, out[0], out[1])


def test_capacity_is_refused_without_a_write():
    cfg, dec = R.TINY, decoder("TINY")
    B, cap = 2, 15
    toks, prompt = R.inputs(cfg, B, 6, 10)
    embs = dec.embed(toks.cuda(), prompt.cuda())
    state = dec.new_state(B, cap, max_steps=4)
    dec.forward(embs[:, :cap], state=state)
    torch.cuda.synchronize()
    before = state.buf.clone()
    with pytest.raises(ValueError):
        dec.forward(embs[:, cap:], state=state)                       # the host's refusal
    nat = state.nat
    ws = state.workspace(1)
    one = embs[:, cap:].contiguous()
    out = torch.empty(B, 1, cfg.vocab_size, device="cuda")
    rc = nat.lib.ac_lm_forward(nat.h, _native._ptr(state.buf), state.buf.numel(), B, cap, 4, cap, _native._ptr(one), 1, _native._ptr(out), None, _native._ptr(ws),
                               ws.numel(), _native._stream())
    assert rc < 0 and b"capacity" in nat.lib.ac_last_error(nat.h)     # the library's refusal
    torch.cuda.synchronize()
    assert state.pos == cap and torch.equal(state.buf, before)
    # a generated token whose row would be position cap + 1: the step records the token, writes no row and raises the flag
    key = int(prng.key_for(0, "sample"))
    for _ in range(2):
        rc = nat.lib.ac_lm_step(nat.h, _native._ptr(state.buf), state.buf.numel(), B, cap, 4, -1, 1.0, 0.0, key, None, _native._ptr(ws), ws.numel(), _native._stream())
        _native.check(rc, nat.h, "ac_lm_step")
    torch.cuda.synchronize()
    hdr = state.header().cpu()
    assert int(hdr[0]) == cap and int(hdr[4]) == 1 and int(hdr[2]) == 1 and int(hdr[3]) == 0
    lay = state.layout
    assert torch.equal(state.buf[lay.kv:], before[lay.kv:]) and torch.equal(state.buf[lay.logits:lay.hyp], before[lay.logits:lay.hyp])
    assert torch.equal(state.hyp()[:, 0].cpu(), state.logits(cfg.vocab_size).argmax(dim=-1).cpu())
    with pytest.raises(_native.NativeError):                          # the host turns the flag into an error at its poll
        state.check()
