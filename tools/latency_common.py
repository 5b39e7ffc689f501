"""What the metrics' `*_latency.py` tools share: the host-clocked call, the alternation of forms on the same data, the median / p99 of
a form, the shader clock and the JSON line."""
import json
import os
import re
import subprocess
import time

import numpy as np
import torch


def shader_mhz():
    """The shader clock, to be sampled while calls are queued; None where the platform reports none."""
    try:
        return round(torch.cuda.clock_rate(), 0)
    except Exception:
        pass
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks", "-d", str(torch.cuda.current_device())], capture_output=True, text=True, timeout=20).stdout
        m = re.search(r"sclk clock level:.*?\((\d+)Mhz\)", txt)
        return float(m.group(1)) if m else None
    except Exception:
        return None


def host_timed(fn, sync=True):
    """Milliseconds on the host clock from an idle device to fn's return and, with `sync`, to the device being idle again (a form that
    ends on the host needs no second synchronisation)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(forms, calls, sync=True):
    """Runs the forms (name -> callable) on alternating calls -- same clocks, same cache state -- for as long as any has calls left
    (`calls`: name -> count).  Returns (name -> list of ms, name -> the last result)."""
    lat, last = {name: [] for name in forms}, {}
    for i in range(max(calls.values())):
        for name, fn in forms.items():
            if i < calls[name]:
                lat[name].append(host_timed(lambda: last.__setitem__(name, fn()), sync))
    return lat, last


def alternate_for(forms, least_calls, window, max_calls, warmup):
    """`alternate` with one count for all forms: `least_calls`, or as many as keep the fastest form busy for `window` seconds (judged
    from `warmup` untimed rounds), at most `max_calls`.  Returns (name -> list of ms, name -> the last result, the count)."""
    warm, _ = alternate(forms, dict.fromkeys(forms, warmup))
    calls = min(max_calls, max(least_calls, int(window * 1e3 / min(min(v) for v in warm.values())) + 1)) if warmup > 0 else least_calls
    return (*alternate(forms, dict.fromkeys(forms, calls)), calls)


def median_p99(ms, digits=3, prefix=""):
    return {f"{prefix}median_ms": round(float(np.median(ms)), digits), f"{prefix}p99_ms": round(float(np.percentile(ms, 99)), digits)}


def emit(row, out=None):
    """One JSON line to stdout and, with `out`, appended to that file."""
    line = json.dumps(row)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")
