"""bench.py --dump-outputs DIR: after the timed steps, the arrays the last timed step handed its caller land in DIR as .npy files
(float32 / float64, at most 64 MB, a fixed seeded sample of a larger array).  Executed without a GPU: the --backend gloo flow with
the stub codec of tests/bench_flow_child.py, and dump_outputs() itself on an array over the whole-array size."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_dump_outputs_writes_the_last_steps_arrays(tmp_path):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env["MASTER_PORT"] = str(_free_port())
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2",
                        "--seconds", "0.5", "--backend", "gloo", "--dump-outputs", str(out)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["dumped_outputs"] == {"toks.npy": [2, 38, 8], "sig.npy": [2, 12160]}
    assert sorted(os.listdir(out)) == ["sig.npy", "toks.npy"]
    toks, sig = np.load(out / "toks.npy"), np.load(out / "sig.npy")
    assert toks.dtype == np.float64 and sig.dtype == np.float32
    # the stub's tokens (rank 0): arange over [B, N, K] modulo the codebook size
    assert np.array_equal(toks, (np.arange(2 * 38 * 8).reshape(2, 38, 8) % 1024).astype(np.float64))
    assert not sig.any()


def test_dump_outputs_samples_a_large_array_reproducibly(tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    big = torch.arange(bench.DUMP_WHOLE_BYTES // 4 + 1024, dtype=torch.float32).reshape(-1, 1024)    # one row over the whole-array size
    small = torch.arange(24, dtype=torch.int64).reshape(2, 3, 4)
    got = []
    for run in ("a", "b"):
        files = bench.dump_outputs(str(tmp_path / run), {"toks": small, "sig": big})
        assert files == {"toks.npy": [2, 3, 4], "sig.npy": [bench.DUMP_SAMPLE], "sig_sample_index.npy": [bench.DUMP_SAMPLE]}
        got.append({f: np.load(tmp_path / run / f) for f in files})
    a, b = got
    for f in a:
        assert np.array_equal(a[f], b[f]), f
    idx = a["sig_sample_index.npy"]
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < big.numel()
    assert np.array_equal(a["sig.npy"], big.reshape(-1).numpy()[idx.astype(np.int64)])
    assert a["toks.npy"].dtype == np.float64 and np.array_equal(a["toks.npy"], small.numpy())
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
