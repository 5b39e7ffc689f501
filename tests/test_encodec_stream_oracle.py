"""The yardstick of the EnCodec stream tests, on the CPU: with the fp64 oracle, the encoder's features and the decoder's samples of a
PREFIX of n >= 7 whole frames equal the first n frames of the whole clip's, and at n = 6 they do not -- the k = 7 frame-rate conv of
each direction then falls under the reference's small-input reflect rule.  Hence a stream that holds back its first 7 frames has the
one-shot result as the oracle of every push schedule, and 7 is the smallest hold that does."""
import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from encodec_stream_cases import HOP, WARMUP, case_of
from golden_cases import make_input, noise

CFGS = [("full", "full_noise_b2"), ("tiny", None)]      # (the tiny fixtures are shorter than 24 frames: seeded noise instead)


@pytest.fixture(scope="module")
def setup(checkpoints):
    from oracle import encodec_oracle as O

    out = {}
    for cfg_name, case in CFGS:
        cfg, sd = checkpoints(cfg_name, 0)
        W64 = O.fold_weight_norm(sd, torch.float64)
        sig = (make_input(case_of(case), GOLDEN_DIR)["sig"] if case else noise(43, 2, 24 * HOP))[:, : 24 * HOP].double()
        assert sig.shape[1] == 24 * HOP
        with torch.no_grad():
            feats = O.sig_to_feats(cfg, W64, sig)
            toks = O.sig_to_toks(cfg, W64, sig)
            rec = O.toks_to_sig(cfg, W64, toks)
        out[cfg_name] = (cfg, W64, sig, feats, toks, rec)
    return out


def test_warmup_is_the_widest_frame_rate_conv(setup):
    for cfg, *_ in setup.values():
        assert max(cfg.kernel_size, cfg.last_kernel_size) == WARMUP and cfg.hop_length == HOP


@pytest.mark.parametrize("cfg_name", [c for c, _ in CFGS])
@pytest.mark.parametrize("n", [7, 8, 20])
def test_prefix_equals_the_whole_clip_from_seven_frames(cfg_name, n, setup):
    from oracle import encodec_oracle as O

    cfg, W64, sig, feats, toks, rec = setup[cfg_name]
    with torch.no_grad():
        f = O.sig_to_feats(cfg, W64, sig[:, : n * HOP])
        r = O.toks_to_sig(cfg, W64, toks[:, :n])
    ef = float((f - feats[:, :n]).abs().max())
    er = float((r - rec[:, : n * HOP]).abs().max())
    print(f"{cfg_name} n={n}: prefix error encode {ef:.2e}, decode {er:.2e}")
    assert f.shape == feats[:, :n].shape and r.shape == rec[:, : n * HOP].shape
    assert ef <= 1e-12 and er <= 1e-12, (ef, er)


@pytest.mark.parametrize("cfg_name", [c for c, _ in CFGS])
def test_six_frames_are_too_few(cfg_name, setup):
    """Nobody lowers the warm-up: at n = 6 both directions visibly differ from the whole clip."""
    from oracle import encodec_oracle as O

    cfg, W64, sig, feats, toks, rec = setup[cfg_name]
    n = WARMUP - 1
    with torch.no_grad():
        f = O.sig_to_feats(cfg, W64, sig[:, : n * HOP])
        r = O.toks_to_sig(cfg, W64, toks[:, :n])
    ef = float((f - feats[:, :n]).abs().max())
    er = float((r - rec[:, : n * HOP]).abs().max())
    print(f"{cfg_name} n={n}: prefix error encode {ef:.2e}, decode {er:.2e}")
    assert ef > 1e-3 and er > 1e-3, (ef, er)


@pytest.mark.parametrize("cfg_name", [c for c, _ in CFGS])
def test_a_partial_last_frame_changes_only_itself(cfg_name, setup):
    from oracle import encodec_oracle as O

    cfg, W64, sig, feats, toks, rec = setup[cfg_name]
    T = 20 * HOP + 137
    with torch.no_grad():
        f = O.sig_to_feats(cfg, W64, sig[:, :T])
    assert f.shape[1] == 21
    e = float((f[:, :20] - feats[:, :20]).abs().max())
    print(f"{cfg_name}: whole frames of a clip with a partial last frame differ by {e:.2e}")
    assert e <= 1e-12, e
    assert float((f[:, 20] - feats[:, 20]).abs().max()) > 1e-6      # the partial frame itself is another frame
