"""bench.py --full: a plain run does only what its headline needs (set-up, warm-ups, the timed steps, --dump-outputs, the line); the
CPU baseline and every other untimed extra run only with --full.  Executed without a GPU: run() in this process with the stub codec of
tests/bench_flow_child.py, no process group, and cpu_baseline() replaced by a recorder."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _run(monkeypatch, capsys, extra):
    import bench
    from audiocodecs_amd.config import ENCODEC_24KHZ as cfg
    from bench_flow_child import StubCodec

    seen = []
    monkeypatch.setattr(bench, "cpu_baseline", lambda *a: seen.append(a[0]) or {"value": 1.0})
    args = bench.parse_args(["--steps", "3", "--warmup", "1", "--batch", "2", "--seconds", "0.5"] + extra)
    sig = torch.zeros(2, 12000)
    codec = StubCodec(0)
    assert bench.run(args, codec, cfg, {}, sig, sig, 0, 1, None, torch.device("cpu")) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), codec.calls, seen


def test_full_is_off_by_default():
    import bench

    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


def test_plain_run_skips_the_extras(monkeypatch, capsys):
    d, calls, seen = _run(monkeypatch, capsys, [])
    assert calls == 2 * 3 + 1            # warm-up + the profiled K steps + the plain K steps, nothing after them
    assert seen == [] and "cpu_baseline" not in d and d["parity"] is None
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "kernels"):
        assert key in d, key
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0


def test_full_run_adds_the_cpu_baseline(monkeypatch, capsys):
    d, calls, seen = _run(monkeypatch, capsys, ["--full"])
    assert calls == 2 * 3 + 1            # (the GPU-only extras do not run on CPU tensors)
    assert seen == ["encodec"] and d["cpu_baseline"] == {"value": 1.0}
    d, _, seen = _run(monkeypatch, capsys, ["--full", "--no-cpu-baseline"])
    assert seen == [] and "cpu_baseline" not in d
