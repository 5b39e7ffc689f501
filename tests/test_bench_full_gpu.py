"""bench.py on the GPU, plain and with --full: the plain line carries the headline and the timed steps' roofline and nothing measured
after them; --full adds the parity gate, the speech-like input, the shader clock and the exact-product twin (the CPU baseline, the other
configs and the latency table are dropped here by their --no-* options to keep the run short).  Small batch: this checks what runs, not
how fast."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("cpu_baseline", "speech_like_ms_per_step", "latency", "exact_fp32_ms_per_step", "exact_fp32_parity", "other_configs")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--seconds", "1"] + list(extra), env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_bench_lines():
    plain = _bench()
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["roofline"]["kernel"] and plain["kernels"]
    assert plain["parity"] is None and "tap_gemm_shader_clock_mhz" not in plain["roofline"]
    assert not [k for k in EXTRAS if k in plain]

    full = _bench("--full", "--no-cpu-baseline", "--no-other-configs", "--no-latency")
    assert full["parity"]["token_mismatches_outside_fp64_near_ties"] == 0
    assert full["parity"]["decode_rms_err"] <= full["parity"]["decode_rms_bar"]
    assert full["speech_like_ms_per_step"] > 0 and "tap_gemm_shader_clock_mhz" in full["roofline"]
    assert full["exact_fp32_ms_per_step"] > 0 and full["exact_fp32_parity"]["token_mismatches_outside_fp64_near_ties"] == 0
    assert not [k for k in ("cpu_baseline", "latency", "other_configs") if k in full]
