#!/usr/bin/env python3
"""Time of one `TokenProbe.forward` against the same modules in torch, on one GPU.

    python tools/token_probe_latency.py [--batches 1 8 64 --frames 750 --calls 10 --warmup 2 --forms probe torch] [--out FILE.jsonl]

The recipe model with seeded random weights (tests/token_probe_ref.py): EnCodec tokens at K = 2 codebooks of C = 1024, E = 128, a two-layer
bidirectional LSTM of H = 512, a CTC head of 1001 classes; N = 750 frames (a 10 s clip), lengths spread between N / 2 and N.  One process,
one JSON line per batch size; the forms run on alternating calls (latency_common), each timed on the host clock from an idle device to an
idle device, `--calls` timed calls behind `--warmup` untimed ones:
    probe   `TokenProbe.forward(toks, lengths)`: frame_pred, hyp_toks and hyp_lens on the device;
    torch   `nn.Embedding` + the pooling + `nn.LSTM` on packed sequences (MIOpen) + `Linear` + `log_softmax` + arg-max in fp32 on the same
            GPU -- without the collapse, which the recipes run on the host.
Each line also carries the share of frames on which the two forms' arg-maxes agree.  Reported, not gated: there is no threshold."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import token_probe_ref as PR  # noqa: E402
from audiocodecs_amd import TokenProbe  # noqa: E402
from latency_common import alternate, emit, median_p99  # noqa: E402

CFG = PR.RECIPE


class TorchProbe(torch.nn.Module):
    """The recipe's modules as torch runs them on the GPU."""

    def __init__(self, cfg, sd):
        super().__init__()
        self.cfg = cfg
        self.emb = torch.nn.Embedding(cfg.table_rows, cfg.embedding_dim)
        self.pool = torch.nn.Linear(cfg.num_codebooks, 1, bias=False)
        self.rnn = torch.nn.LSTM(cfg.embedding_dim, cfg.hidden_size, cfg.num_layers, batch_first=True, bidirectional=True)
        self.head = torch.nn.Linear(2 * cfg.hidden_size, cfg.num_classes)
        with torch.no_grad():
            self.emb.weight.copy_(sd["embedding.weight"])
            self.pool.weight.copy_(sd["pooling.mlp.weight"])
            for name, p in self.rnn.named_parameters():
                p.copy_(sd["encoder.rnn." + name])
            self.head.weight.copy_(sd["head.weight"])
            self.head.bias.copy_(sd["head.bias"])
        self.offsets = torch.arange(0, cfg.num_codebooks * cfg.vocab_size, cfg.vocab_size)

    @torch.no_grad()
    def forward(self, toks, lengths_host):
        x = self.emb(toks + self.offsets.to(toks.device))
        x = self.pool(x.movedim(-1, -2))[..., 0]
        pk = torch.nn.utils.rnn.pack_padded_sequence(x, lengths_host, batch_first=True, enforce_sorted=False)
        y = torch.nn.utils.rnn.pad_packed_sequence(self.rnn(pk)[0], batch_first=True, total_length=toks.shape[1])[0]
        return torch.log_softmax(self.head(y), dim=-1).argmax(dim=-1)


def measure(B, a, probe, ref):
    g = torch.Generator().manual_seed(B)
    N = a.frames
    toks = torch.randint(0, CFG.vocab_size, (B, N, CFG.num_codebooks), generator=g).cuda()
    lengths_host = torch.randint(N // 2, N + 1, (B,), generator=g)
    lengths_host[0] = N
    lengths = lengths_host.cuda()
    forms = {k: v for k, v in {"probe": lambda: probe.forward(toks, lengths).frame_pred, "torch": lambda: ref(toks, lengths_host)}.items() if k in a.forms}
    alternate(forms, dict.fromkeys(forms, a.warmup))
    lat, last = alternate(forms, dict.fromkeys(forms, a.calls))
    row = {"what": "token_probe", "B": B, "N": N, "calls": a.calls, "forms": list(forms)}
    for k in forms:
        row.update(median_p99(lat[k], 3, k + "_"))
    if len(forms) == 2:
        valid = torch.arange(N, device="cuda")[None, :] < lengths[:, None]
        row["pred_equal"] = round(float((last["probe"][valid] == last["torch"][valid]).double().mean()), 6)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=750)
    ap.add_argument("--calls", type=int, default=10, help="timed calls per form and batch size")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--forms", nargs="+", default=["probe", "torch"], choices=["probe", "torch"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("token_probe_latency: no GPU: a timing needs one")
    sd = PR.weights(CFG)
    probe = TokenProbe(state_dict=sd, config=CFG)
    ref = TorchProbe(CFG, sd).cuda() if "torch" in a.forms else None
    for B in a.batches:
        emit(measure(B, a, probe, ref), a.out)


if __name__ == "__main__":
    main()
