#!/usr/bin/env python3
"""Call latency of `dnsmos` against the same chain as torch ops on the GPU and against the reference's regime restated, on one GPU.

    python tools/dnsmos_latency.py [--clips 64 --calls 30 --torch-calls 10 --host-calls 1 --warmup 3] [--out profiles/dnsmos_latency.jsonl]

One process; `clips` x 10 s at 24 kHz (at 16 kHz a clip of 160000 samples has one window of 9.01 s).  Three forms run on the SAME data on
alternating calls (same clocks, same cache state) for as long as any form has calls left:
    fused    `dnsmos(sig, 24000, weights)`: the library's resampler, then ac_dnsmos; nothing leaves the device but the scores
    torch    the same chain as torch fp32 ops on the same GPU: the library's resampler, torch.stft (n_fft 321), the filterbank as a matmul,
             the dB rule, F.conv2d / F.max_pool2d / amax / matmul, all windows as one batch
    host     downstream/metrics/dnsmos.py restated: the library's resampler on the device (torchaudio is not installed), the signals moved
             to the host, then clip by clip, in a Python loop, the fp64 numpy / torch statement (tests/dnsmos_ref.py: librosa and
             onnxruntime are not installed; they do the same steps, each window on its own)
Every call is timed on the host from the call to the scores being on the host.  One JSON line: median / p99 (ms) of each form, the largest
absolute difference of the fused scores from the other two and the shader clock sampled while calls are queued (None where the platform
reports none).  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiocodecs_amd import dnsmos, dnsmos_segments  # noqa: E402
from audiocodecs_amd.dnsmos import load_weights  # noqa: E402
from audiocodecs_amd.resample import resample  # noqa: E402
from latency_common import alternate, emit, median_p99, shader_mhz  # noqa: E402

RATE = 24000
SECONDS = 10


class TorchChain:
    """The chain as torch fp32 ops on the device, all windows of all clips as one batch."""

    def __init__(self, weights, R, device):
        self.w = {k: v.to(device) for k, v in weights.tensors.items()}
        self.fb = torch.from_numpy(R.filterbank().astype(np.float32)).to(device)
        self.win = torch.hann_window(321, periodic=True, device=device)

    def __call__(self, sig):
        F = torch.nn.functional
        x = resample(sig, RATE, 16000)
        starts = dnsmos_segments(int(x.shape[1]))
        assert int(x.shape[1]) >= 144160                                # (no doubling in this tool's shape)
        wins = torch.stack([x[:, s:s + 144000] for s in starts], dim=1).reshape(-1, 144000)
        S = torch.stft(wins, n_fft=321, hop_length=160, window=self.win, center=True, pad_mode="constant", return_complex=True).abs().pow(2)
        mel = S.transpose(1, 2) @ self.fb                               # [N, 900, 120]
        db = 10.0 * torch.log10(mel.clamp_min(1e-10))
        db = db - db.amax(dim=(1, 2), keepdim=True)
        h = ((db.clamp_min(-80.0) + 40.0) / 40.0).unsqueeze(1)
        w = self.w
        h = F.max_pool2d(F.relu(F.conv2d(h, w["conv5.w"], w["conv5.b"], padding=1)), 2)
        h = F.max_pool2d(F.relu(F.conv2d(h, w["conv6.w"], w["conv6.b"], padding=1)), 2)
        h = F.relu(F.conv2d(h, w["conv7.w"], w["conv7.b"], padding=1))
        h = F.max_pool2d(F.relu(F.conv2d(h, w["conv8.w"], w["conv8.b"], padding=1)), 2)
        h = F.relu(F.conv2d(h, w["conv9.w"], w["conv9.b"], padding=1)).amax(dim=(2, 3))
        h = F.relu(h @ w["dense3.w"] + w["dense3.b"])
        h = F.relu(h @ w["dense4.w"] + w["dense4.b"])
        return (h @ w["dense5.w"] + w["dense5.b"]).reshape(x.shape[0], len(starts)).mean(dim=1)


def host_regime(sig, R):
    x = resample(sig, RATE, 16000).cpu().numpy()
    return np.array([R.score_clip(c)[0] for c in x])


def main():
    import dnsmos_ref as R

    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--calls", type=int, default=30, help="timed calls of the fused form")
    ap.add_argument("--torch-calls", type=int, default=10, help="timed calls of the torch-on-GPU form")
    ap.add_argument("--host-calls", type=int, default=1, help="timed calls of the host form (tens of seconds each at 64 clips)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of the fused and the torch form")
    ap.add_argument("--weights", default=os.path.join(ROOT, "tests", "golden", "dnsmos_p808.npz"))
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    weights = load_weights(a.weights)
    B, T = a.clips, SECONDS * RATE
    sig = torch.from_numpy(np.stack([R.make_signal(R.KINDS[b % 3], T, seed=b) for b in range(B)])).cuda()
    chain = TorchChain(weights, R, sig.device)
    for _ in range(a.warmup):
        dnsmos(sig, RATE, weights).cpu()
        chain(sig).cpu()
    forms = {"fused": lambda: dnsmos(sig, RATE, weights).cpu(), "torch": lambda: chain(sig).cpu(), "host": lambda: host_regime(sig, R)}
    lat, last = alternate(forms, {"fused": a.calls, "torch": a.torch_calls, "host": a.host_calls}, sync=False)      # (every form ends on the host)
    fused, tch, host = (last.get(name) for name in forms)
    row = {"clips": B, "seconds": SECONDS, "rate": RATE, "windows": B * len(dnsmos_segments(SECONDS * 16000)), "calls": a.calls, "torch_calls": a.torch_calls,
           "host_calls": a.host_calls, "warmup": a.warmup}
    for name, v in lat.items():
        if v:
            row.update(median_p99(v, prefix=f"{name}_"))
    for _ in range(5):
        dnsmos(sig, RATE, weights)
    row["shader_mhz"] = shader_mhz()
    torch.cuda.synchronize()
    if tch is not None:
        row["largest_difference_from_torch"] = float((fused.double() - tch.double()).abs().max())
    if host is not None:
        row["largest_difference_from_host"] = float(np.abs(fused.numpy().astype(np.float64) - host).max())
    emit(row, a.out)


if __name__ == "__main__":
    main()
