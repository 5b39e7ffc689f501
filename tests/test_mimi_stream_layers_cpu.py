"""The fp64 statement of one streamed Mimi sub-layer (tests/mimi_stream_layer_ref.py), checked alone: no kernel runs here.

tests/test_mimi_stream_layers_gpu.py holds every tap of a Mimi stream push to `ref64 = sub_layer(the GPU's own earlier taps)` under
the per-tap bar  |err| <= 5e-6 * max(1, max|ref64|) + 2e-5 * |ref64|.  That is only worth something if

  1. ref64 is right: chaining qkv_rot -> attend -> layer_out over a push schedule (and `upsample` over the decode pushes) equals
     `mimi_oracle.transformer_layer` (`mimi_oracle.upsample`) run one-shot over the whole sequence in fp64, to 1e-12 relative;
  2. a correct fp32 kernel has room: the same functions in fp32 (`ref32`), on the fp32-rounded inputs of ref64, stay within 0.5 of
     the bar on every sub-layer tap of every push of every case;
  3. the faults specific to the streamed attention do NOT fit under the bar: a window of one key fewer or more, a ring read one
     slot off (either way), a history missing the previous push (one push stale: the slots still hold what was there a ring earlier, or
     zeros), the neighbouring stream's history, a push placed one position off -- each puts at least one element of EVERY affected
     row more than 10 times past the bar, in every layer of every push.  So the GPU test fails for each of them.

The cases are those of the GPU test, seen per stream (a slot push is, to one stream, a push like any other): the full config's
lockstep schedule across the window of 250 and the ring of 249, the tiny config (window 6, ring 5, head_dim 16) with B = 3, the
two sessions of the slot case (one to position 300 and on, one from 0) and the two of the stale-ring case.  The transformer's input
is the fp32 oracle's: the SEANet encoder's output of the case's signal (encode), the streamed up-sampler's output of the oracle's
tokens of that signal (decode).

Measured (largest ref32 |err| / bar over all pushes and layers, qkv / att / out / up-sampler): full config 0.097 / 0.077 / 0.059 /
0.004, tiny config 0.033 / 0.030 / 0.032 / 0.003 -- no case needed another signal.  Least excess of an affected row over the bar:
full config 145 x (window + 1), 162 x (window - 1), 183 x (a push taken one position early, in the attention), 248 x (ring slot
off), 618 x (previous push missing), 21750 x (neighbour's history), 32649 x (RoPE one position off); tiny config 4696 x and up."""
import pytest
import torch

import mimi_stream_layer_cases as MC
import mimi_stream_layer_ref as R
from oracle import mimi_oracle as O

# (case, config, [(stream name, signal seed, B, frames per push)])
CASES = [
    ("full_lockstep", "full", [("s", MC.SEED["full"], 1, MC.FULL_FRAMES)]),
    ("tiny_lockstep", "tiny", [("s", MC.SEED["tiny"], 3, MC.TINY_FRAMES)]),
    ("slots_full", "full", [("slot0", MC.SEED["slot0"], 1, MC.SLOT_ALONE_FRAMES + [f for _, f in MC.SLOT_JOINT]),
                            ("slot2", MC.SEED["slot2"], 1, [f for _, f in MC.SLOT_JOINT])]),
    ("stale_tiny", "tiny", [("slot0", MC.SEED["stale0"], 1, MC.STALE_FIRST_FRAMES + MC.STALE_SECOND_FRAMES),
                            ("slot1", MC.SEED["stale1"], 1, MC.STALE_SECOND_FRAMES)]),
]
PARAMS = [(c[0], d) for c in CASES for d in ("encode", "decode")]
IDS = [f"{c}-{d}" for c, d in PARAMS]

_W, _RUN = {}, {}


def _weights(cfg_name, mimi_checkpoints):
    if cfg_name not in _W:
        cfg, sd = mimi_checkpoints(cfg_name, 0)
        _W[cfg_name] = (cfg, O.cast_weights(sd), O.cast_weights(sd, torch.float64))
    return _W[cfg_name]


def _streams(case, direction, mimi_checkpoints):
    """Per stream of the case: the fp64 chain over its schedule.  -> (cfg, W, W64, part, [stream dict])."""
    torch.set_num_threads(min(16, max(1, torch.get_num_threads())))
    _, cfg_name, groups = next(c for c in CASES if c[0] == case)
    cfg, W, W64 = _weights(cfg_name, mimi_checkpoints)
    part = MC.PARTS[direction]
    if (case, direction) not in _RUN:
        out = []
        for name, seed, B, frames in groups:
            run = MC.oracle_run((cfg_name, seed, B, sum(frames)), cfg, W, MC.signal(seed, B, sum(frames)))
            s = {"name": name, "B": B, "frames": frames, "sizes": MC.rows_of(frames, cfg.resample_stride)}
            with torch.no_grad():
                if direction == "encode":
                    x = run["x_enc"].double()
                else:
                    qf = O.rvq_decode(cfg, W64, run["toks"].movedim(-1, -2)).transpose(1, 2)        # [B,N,H]
                    s["qf"] = qf
                    ups, prev = [], None
                    for q in torch.split(qf, frames, 1):
                        ups.append(R.upsample(cfg, W64, prev, q))
                        prev = q[:, -1]
                    x = torch.cat(ups, 1)
                s["x"] = x
                s["taps"], s["kh"], s["vh"] = R.chain(cfg, W64, part, MC.split_rows(x, s["sizes"]))
            out.append(s)
        _RUN[case, direction] = out
    return cfg, W, W64, part, _RUN[case, direction]


@pytest.mark.parametrize("case,direction", PARAMS, ids=IDS)
def test_the_chained_sub_layers_are_the_one_shot_layer(case, direction, mimi_checkpoints):
    cfg, W, W64, part, streams = _streams(case, direction, mimi_checkpoints)
    for s in streams:
        with torch.no_grad():
            if direction == "decode":
                want = O.upsample(cfg, W64)[1](s["qf"].transpose(1, 2)).transpose(1, 2)
                assert float((s["x"] - want).abs().max()) <= 1e-12 * float(want.abs().max()), f"{case}/{s['name']}: up-sampler"
            y = s["x"]
            for l in range(cfg.num_hidden_layers):
                y = O.transformer_layer(cfg, W64, f"{part}.layers.{l}", y)
                got = torch.cat([t[l]["out"] for t in s["taps"]], 1)
                err = float((got - y).abs().max()) / float(y.abs().max())
                assert err <= 1e-12, f"{case}/{s['name']} layer {l}: chained {err:.2e} relative off the one-shot layer"


def _over_bar(got, ref64):
    return (got.double() - ref64).abs() / MC.bar(ref64)


@pytest.mark.parametrize("case,direction", PARAMS, ids=IDS)
def test_the_fp32_restatement_has_headroom_under_the_bar(case, direction, mimi_checkpoints):
    """ref32 against ref64 on the SAME fp32-rounded inputs, as the GPU test computes the two."""
    cfg, W, W64, part, streams = _streams(case, direction, mimi_checkpoints)
    A = cfg.num_attention_heads * cfg.head_dim
    worst = {"qkv": 0.0, "att": 0.0, "out": 0.0, "upsample": 0.0}
    with torch.no_grad():
        for s in streams:
            if direction == "decode":
                prev = None
                for q in torch.split(s["qf"].float(), s["frames"], 1):
                    r64 = R.upsample(cfg, W64, None if prev is None else prev.double(), q.double())
                    worst["upsample"] = max(worst["upsample"], float(_over_bar(R.upsample(cfg, W, prev, q), r64).max()))
                    prev = q[:, -1]
            for i, push in enumerate(s["taps"]):
                for l, t in enumerate(push):
                    x, qkv, att, p0 = t["in"].float(), t["qkv"].float(), t["att"].float(), t["pos0"]
                    kh, vh = s["kh"][l][:, :p0].float(), s["vh"][l][:, :p0].float()
                    q, k, v = qkv[..., :A], qkv[..., A:2 * A], qkv[..., 2 * A:]
                    pairs = {
                        "qkv": (R.qkv_rot(cfg, W, l, part, x, p0), R.qkv_rot(cfg, W64, l, part, x.double(), p0)),
                        "att": (R.attend(cfg, q, kh, vh, k, v, p0), R.attend(cfg, q.double(), kh.double(), vh.double(), k.double(), v.double(), p0)),
                        "out": (R.layer_out(cfg, W, l, part, x, att), R.layer_out(cfg, W64, l, part, x.double(), att.double())),
                    }
                    for name, (r32, r64) in pairs.items():
                        assert r32.dtype == torch.float32 and r64.dtype == torch.float64
                        ratio = float(_over_bar(r32, r64).max())
                        worst[name] = max(worst[name], ratio)
                        assert ratio <= 0.5, f"{case}/{direction}/{s['name']} push {i} layer {l} {name}: ref32 at {ratio:.3f} of the bar"
    print(f"{case} {direction}: worst ref32 |err|/tol " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert worst["upsample"] <= 0.5, worst


def _neighbour_hist(streams, si, l, p0):
    """The history another stream of the case holds at the same positions (zeros where it holds nothing): the next batch row of a
    lockstep stream, the other session of a slot case."""
    s = streams[si]
    if s["B"] > 1:
        return s["kh"][l][:, :p0].roll(1, 0), s["vh"][l][:, :p0].roll(1, 0)
    o = streams[(si + 1) % len(streams)]
    out = []
    for h in (o["kh"][l], o["vh"][l]):
        z = torch.zeros(1, p0, h.shape[-1], dtype=h.dtype)
        n = min(p0, h.shape[1])
        z[:, :n] = h[:, :n]
        out.append(z)
    return out


@pytest.mark.parametrize("case,direction", PARAMS, ids=IDS)
def test_the_bar_catches_the_faults_of_the_streamed_attention(case, direction, mimi_checkpoints):
    cfg, W, W64, part, streams = _streams(case, direction, mimi_checkpoints)
    A, win = cfg.num_attention_heads * cfg.head_dim, cfg.sliding_window
    ring = win - 1
    least, seen = {}, set()

    def check(what, where, pert, ref, affected):
        if not bool(affected.any()):
            return
        over = _over_bar(pert, ref).amax(-1)[:, affected]            # [B, affected rows]: the worst element of each row
        least[what] = min(least.get(what, float("inf")), float(over.min()))
        seen.add(what)
        assert float(over.min()) > 10, f"{where}: {what} leaves a row within {float(over.min()):.2f} x the bar"

    with torch.no_grad():
        for si, s in enumerate(streams):
            for i, push in enumerate(s["taps"]):
                for l, t in enumerate(push):
                    where = f"{case}/{direction}/{s['name']} push {i} layer {l}"
                    qkv, att, p0 = t["qkv"], t["att"], t["pos0"]
                    T = qkv.shape[1]
                    q, k, v = qkv[..., :A], qkv[..., A:2 * A], qkv[..., 2 * A:]
                    kh, vh = s["kh"][l][:, :p0], s["vh"][l][:, :p0]
                    pos = p0 + torch.arange(T)
                    sees_hist = (torch.arange(T) <= win - 2) & (p0 >= 1)          # the query sees position p0 - 1
                    check("window - 1", where, R.attend(cfg, q, kh, vh, k, v, p0, window=win - 1), att, pos >= win - 1)
                    check("window + 1", where, R.attend(cfg, q, kh, vh, k, v, p0, window=win + 1), att, pos >= win)
                    if p0 >= 1:
                        # The ring before this push: slot j % R holds position j for the last R positions (zeros where nothing was
                        # written).  Read one slot off, a query that sees n of the R slots sees another set of rows unless n = R
                        # (row 0 of a push behind a full ring: the same rows in another order, which the softmax does not notice).
                        j = torch.arange(max(0, p0 - ring), p0)
                        n_seen = p0 - (pos - win + 1).clamp(min=0)
                        off_rows = (n_seen >= 1) & (n_seen < ring)
                        for d in (1, -1):
                            ks, vs = kh.clone(), vh.clone()
                            for h, hs in ((kh, ks), (vh, vs)):
                                slots = torch.zeros(h.shape[0], ring, A, dtype=h.dtype)
                                slots[:, j % ring] = h[:, j]
                                hs[:, j] = slots[:, (j + d) % ring]
                            check(f"ring read one slot off ({d:+d})", where, R.attend(cfg, q, ks, vs, k, v, p0), att, off_rows)
                    if i >= 1:
                        prev = s["sizes"][i - 1]
                        km, vm = kh.clone(), vh.clone()
                        for j in range(p0 - min(prev, ring), p0):                 # the slots the previous push should have written
                            km[:, j] = kh[:, j - ring] if j >= ring else 0.0
                            vm[:, j] = vh[:, j - ring] if j >= ring else 0.0
                        check("history missing the previous push", where, R.attend(cfg, q, km, vm, k, v, p0), att, sees_hist)
                    if p0 >= 1 and (s["B"] > 1 or len(streams) > 1):
                        kn, vn = _neighbour_hist(streams, si, l, p0)
                        check("the neighbouring stream's history", where, R.attend(cfg, q, kn, vn, k, v, p0), att, sees_hist)
                    if p0 >= 1:    # the push taken for one position earlier: the last history row is not seen, the window starts one lower
                        check("push one position early (attention)", where, R.attend(cfg, q, kh[:, :-1], vh[:, :-1], k, v, p0 - 1), att, sees_hist)
                        check("push one position early (RoPE)", where, R.qkv_rot(cfg, W64, l, part, t["in"], p0 - 1), qkv, pos >= 0)
                    check("push one position late (RoPE)", where, R.qkv_rot(cfg, W64, l, part, t["in"], p0 + 1), qkv, pos >= 0)
    print(f"{case} {direction}: least excess of an affected row over the bar  " + "  ".join(f"{k}: {v:.0f}x" for k, v in least.items()))
    must = {"window - 1", "window + 1", "ring read one slot off (+1)", "ring read one slot off (-1)", "history missing the previous push", "push one position early (attention)",
            "push one position early (RoPE)", "push one position late (RoPE)"}
    if streams[0]["B"] > 1 or len(streams) > 1:
        must.add("the neighbouring stream's history")
    assert must <= seen, must - seen
