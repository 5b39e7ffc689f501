"""The persistent LSTM's recurrent exchange is a ring of LP16_RING = 8 time steps that the kernel re-arms itself (lstm_persist16.h);
only the ring is filled before a launch.  Full-size EnCodec (D = 512: the persistent kernel) at frame counts below, at and across the
ring length and at several wraps, with full and ragged 16-clip groups, against the CPU oracle -- the bars of the smoke run: tokens equal
outside fp64 near-ties, waveform within 1e-5 RMS -- twice per case on one handle: the second run starts from the ring the first one left
(its last slots hold published values, not the fill) and must return the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HOP = 320          # samples per frame (24 kHz, 75 frames per second)
RING = 8           # LP16_RING
# (clips, frames): T < ring, T = ring, one step over, two wraps and a step, many wraps; 17 clips = one full and one 1-clip group
CASES = [(2, 1), (2, 2), (2, 3), (3, RING - 1), (3, RING), (17, RING + 1), (2, 2 * RING + 1), (17, 5 * RING + 3)]


@pytest.fixture(scope="module")
def setup():
    from audiocodecs_amd import Encodec, checkpoint
    from audiocodecs_amd.config import ENCODEC_24KHZ as cfg
    from oracle import encodec_oracle as O

    sd = checkpoint.synthetic_state_dict(cfg, seed=0)
    codec = Encodec(24000, num_codebooks=8, state_dict=sd).eval()
    return cfg, codec, O, O.fold_weight_norm(sd), O.fold_weight_norm(sd, torch.float64)


@pytest.mark.parametrize("B,T", CASES)
def test_ring_exchange_matches_the_oracle_and_itself(setup, B, T):
    from audiocodecs_amd import prng

    cfg, codec, O, W, W64 = setup
    sig = torch.from_numpy((prng.normal(11, f"ring{B}x{T}", (B, T * HOP)) * 0.1).astype(np.float32))
    toks = codec.sig_to_toks(sig.cuda())
    rec = codec.toks_to_sig(toks)
    toks2 = codec.sig_to_toks(sig.cuda())
    rec2 = codec.toks_to_sig(toks2)
    torch.cuda.synchronize()
    assert toks.shape[1] == T
    nat = next(iter(codec._natives.values()))
    assert nat.lib.ac_lstm_status(nat.h) >= 0, "persistent LSTM reported a failed launch"
    assert torch.equal(toks, toks2) and torch.equal(rec, rec2)
    with torch.no_grad():
        otoks = O.sig_to_toks(cfg, W, sig)
        _, m64 = O.sig_to_toks(cfg, W64, sig.double(), None, 8, True)
        orec = O.toks_to_sig(cfg, W, toks.cpu())
    diff = toks.cpu() != otoks
    safe = torch.cumprod((m64 > 1e-4).to(torch.int64), dim=-1).bool()
    bad = int((diff & safe).sum())
    err = float((rec.cpu() - orec).pow(2).mean().sqrt())
    print(f"ring {B} x {T}: {int(diff.sum())}/{diff.numel()} tokens differ ({bad} outside near-ties), waveform RMS err {err:.2e}")
    assert bad == 0 and int(diff.sum()) <= int((~safe).sum()) and err < 1e-5
