"""GPU tests of the WavLM x-vector speaker encoder (audiocodecs_amd.spksim, csrc/wavlm.h, csrc/spk_path.hip) against
the fp64 statement of tests/spksim_ref.py, stage by stage.

Tolerance: a stage's bound is K x the largest error of the SAME statement run in fp32 on the CPU against fp64 over the test's own cases
(computed here, never from the library's output), K = 8: split16 products are fp32-FMA-like, the sums run in another order, exp is
v_exp_f32.  A cosine's bound is K x max(that error of the cosine, 2^-23): one fp32 ulp of a value near 1 is the least an fp32 result can
differ by.  What needs no tolerance is compared exactly: NaN embeddings, the refusal of a clip without a pooled row, and the equality of
a clip's result whatever the batch around it or its chunking."""
import ctypes as C
import dataclasses

import pytest
import torch

import spksim_ref as R
from audiocodecs_amd.spksim import WAVLM_BASE_SV, WAVLM_SV_TINY

pytestmark = pytest.mark.gpu

K = 8
_ENC = {}


def _encoder(cfg=WAVLM_SV_TINY):
    """A SpeakerEncoder of the tiny model's synthetic weights under `cfg` (which may differ from the tiny config in its chunking)."""
    from audiocodecs_amd import SpeakerEncoder

    if cfg not in _ENC:
        _ENC[cfg] = SpeakerEncoder(state_dict=R.tiny_state_dict(), arch=cfg)
    return _ENC[cfg]


def _run(enc, sig, valid=None):
    v = None if valid is None else torch.tensor(valid, dtype=torch.int32).cuda()
    emb, st = enc.embed_16k(sig.cuda(), v, return_stages=True)
    torch.cuda.synchronize()
    out = {k: t.cpu().double() for k, t in st.items()}
    out["emb"] = emb.cpu().double()
    return out


def _compare(tag, got, want, err, stages=R.STAGES, k=K):
    """Every stage within k x the fp32 statement's own error; prints the measured ratio of each before it asserts."""
    worst = {}
    for s in stages:
        nan = torch.isnan(want[s])
        assert torch.equal(torch.isnan(got[s]), nan), (tag, s, "NaN pattern")
        d = float((got[s] - want[s])[~nan].abs().max()) if (~nan).any() else 0.0
        worst[s] = d / err[s] if err[s] > 0 else (0.0 if d == 0 else float("inf"))
        print(f"{tag} {s}: |lib - fp64| = {d:.3e}, |fp32 statement - fp64| = {err[s]:.3e}, ratio {worst[s]:.2f}")
    for s in stages:
        assert worst[s] <= k, (tag, s, worst[s])
    return worst


def _merge(*errs):
    return {s: max(e[s] for e in errs) for s in R.STAGES}


def test_stages_unmasked_and_masked():
    """Four different clips at T = 130 (beyond the bucket clamp at 80, over two key tiles), once unmasked and once with
    valid = [L, 32000, 20560, L]: Lf = 130, 99, 64 (a tile edge); the full-length masked clips hit min(Lf - 8, T - 14)."""
    cfg, sd, enc = WAVLM_SV_TINY, R.tiny_state_dict(), _encoder()
    sig = R.clips(4, R.MAIN_L)
    w0, e0 = R.stage_errors(cfg, sd, sig, None)
    w1, e1 = R.stage_errors(cfg, sd, sig, R.MAIN_VALID)
    assert w1["Lf"] == [130, 99, 64, 130] and w1["rows"] == [116, 91, 56, 116] and w0["rows"] == [116] * 4
    err = _merge(e0, e1)
    _compare("unmasked", _run(enc, sig), w0, err)
    got = _run(enc, sig, R.MAIN_VALID)
    _compare("masked", got, w1, err)
    # the pooled row counts are exact: the same statistics over one row more or fewer lie outside the bound
    for b in (1, 2):
        n = w1["rows"][b]
        for m in (n - 1, n + 1):
            other = torch.cat([w1["tdnn"][b, :m].mean(0), w1["tdnn"][b, :m].std(0)])
            assert float((other - w1["pooled"][b]).abs().max()) > K * err["pooled"], (b, m)
    # masked rows of the projected features are zero before the positional conv: the first hidden state differs from the unmasked one
    assert float((w1["hidden"][0, 2, 64:] - w0["hidden"][0, 2, 64:]).abs().max()) > 1e-3


@pytest.mark.parametrize("T", [16, 63, 64, 65, 129])
def test_attention_seams(T):
    """B = 2 at the key-tile seams; clip 1 is masked to Lf = T - 1.  `hidden` holds every layer's input and the last output."""
    cfg, sd, enc = WAVLM_SV_TINY, R.tiny_state_dict(), _encoder()
    L = R.length_for_frames(T)
    sig = R.clips(2, L, seed=T)
    valid = [L, R.length_for_frames(T - 1)]
    want, err = R.stage_errors(cfg, sd, sig, valid)
    assert want["Lf"] == [T, T - 1] and want["hidden"].shape[2] == T
    _compare(f"T={T}", _run(enc, sig, valid), want, err, stages=("hidden", "emb"))


def test_short_clips():
    """L = 5200: two pooled rows, finite.  L = 4880: one pooled row, std of one row: an all-NaN embedding, as the backend.  L = 4879: no
    row at all, refused by ac_spk_embed."""
    cfg, sd, enc = WAVLM_SV_TINY, R.tiny_state_dict(), _encoder()
    sig = R.clips(2, 5200, seed=3)
    want, err = R.stage_errors(cfg, sd, sig, None)
    assert want["rows"] == [2, 2]
    got = _run(enc, sig)
    assert torch.isfinite(got["emb"]).all()
    _compare("L=5200", got, want, err)
    sig = R.clips(2, 4880, seed=4)
    want = R.forward(cfg, sd, sig, None, torch.float64)
    assert want["rows"] == [1, 1] and torch.isnan(want["emb"]).all()
    got = _run(enc, sig)
    assert torch.isnan(got["emb"]).all() and got["emb"].shape == (2, cfg.xvector_output_dim)
    assert torch.isfinite(got["pooled"][:, : cfg.tdnn_dim[-1]]).all() and torch.isnan(got["pooled"][:, cfg.tdnn_dim[-1]:]).all()
    # a masked clip with one pooled row beside a full one: NaN for that clip only
    sig = R.clips(2, 8000, seed=5)
    valid = [8000, R.length_for_frames(9)]
    want = R.forward(cfg, sd, sig, valid, torch.float64)
    assert want["rows"] == [10, 1]
    got = _run(enc, sig, valid)
    assert torch.isfinite(got["emb"][0]).all() and torch.isnan(got["emb"][1]).all()
    # the library itself refuses a clip too short for one pooled row (the Python wrapper refuses earlier)
    nat = enc._native_for(torch.empty(0, device="cuda"))
    x = torch.zeros(1, 4879, device="cuda")
    emb = torch.empty(1, cfg.xvector_output_dim, device="cuda")
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
    rc = nat.lib.ac_spk_embed(nat.h, C.c_void_p(x.data_ptr()), None, 1, 4879, C.c_void_p(emb.data_ptr()), None, C.c_void_p(ws.data_ptr()), ws.numel(), None)
    assert rc == -1 and b"4879" in nat.lib.ac_last_error(nat.h)


def test_full_width():
    """WAVLM_BASE_SV (the real shape: split16 tap-GEMMs in every conv, the 48-channel x 128-tap positional conv), B = 2, L = 32080, the
    second clip valid to 20000 samples: embeddings and the cosine."""
    from audiocodecs_amd import checkpoint
    from audiocodecs_amd.spksim import cosine

    cfg = WAVLM_BASE_SV
    sd = checkpoint.synthetic_wavlm_sv_state_dict(cfg, 1)
    from audiocodecs_amd import SpeakerEncoder

    enc = SpeakerEncoder(state_dict=sd, arch=cfg)
    L = 32080
    sig = R.clips(2, L, seed=6)
    valid = [L, 20000]
    want, err = R.stage_errors(cfg, sd, sig, valid)
    got = _run(enc, sig, valid)
    _compare("full", got, want, err)
    cos64 = torch.nn.functional.cosine_similarity(want["emb"][:1], want["emb"][1:], dim=-1)
    s32 = R.forward(cfg, sd, sig, valid, torch.float32)
    cos32 = torch.nn.functional.cosine_similarity(s32["emb"][:1], s32["emb"][1:], dim=-1).double()
    e = got["emb"].float().cuda()
    c = cosine(e[:1], e[1:]).cpu().double()
    bound = K * max(float((cos32 - cos64).abs()), 2.0 ** -23)
    print(f"full cosine: lib {float(c):.7f}, fp64 {float(cos64):.7f}, |diff| {float((c - cos64).abs()):.2e}, bound {bound:.2e}")
    assert float((c - cos64).abs()) <= bound


def test_chunking_is_bit_identical():
    """B = 5 with max_chunk_clips = 2 against the automatic chunking, and clip 3 alone against clip 3 in the batch."""
    sig = R.clips(5, 12000, seed=7)
    valid = [12000, 9000, 12000, 7000, 11000]
    auto = _encoder()
    two = _encoder(dataclasses.replace(WAVLM_SV_TINY, max_chunk_clips=2))
    for v in (None, valid):
        a, b = _run(auto, sig, v), _run(two, sig, v)
        for s in R.STAGES:
            assert torch.equal(a[s], b[s]), s
        one = _run(auto, sig[3:4], None if v is None else v[3:4])
        for s in R.STAGES:
            x = a[s][:, 3:4] if s == "hidden" else a[s][3:4]
            assert torch.equal(one[s], x), s


def test_public_path():
    """`speaker_similarity` at 24 kHz against the statement fed the library's own resampled signal; two `append`s and `summarize`;
    `Codec.resynthesis_spk_sim` on a TINY EnCodec equals `speaker_similarity` of its `_resynthesize` output."""
    from audiocodecs_amd import Encodec, SpkSimWavLM, checkpoint, speaker_similarity
    from audiocodecs_amd.config import TINY
    from audiocodecs_amd.resample import resample

    cfg, sd, enc = WAVLM_SV_TINY, R.tiny_state_dict(), _encoder()
    B, T24 = 3, 18000
    ref = R.clips(B, T24, seed=8)
    hyp = R.clips(2 * B, T24, seed=9)[B:]
    lens = torch.tensor([1.0, 0.8, 0.55])
    for ln in (None, lens):
        got = speaker_similarity(hyp.cuda(), ref.cuda(), 24000, enc, None if ln is None else ln.cuda()).cpu().double()
        x16 = resample(torch.cat([hyp, ref]).cuda(), 24000, 16000).cpu()
        L16 = x16.shape[-1]
        valid = None if ln is None else [int(v) for v in (torch.cat([ln, ln]) * L16).int()]
        w64 = R.forward(cfg, sd, x16, valid, torch.float64)["emb"]
        w32 = R.forward(cfg, sd, x16, valid, torch.float32)["emb"]
        c64 = torch.nn.functional.cosine_similarity(w64[:B], w64[B:], dim=-1)
        c32 = torch.nn.functional.cosine_similarity(w32[:B], w32[B:], dim=-1).double()
        bound = K * max(float((c32 - c64).abs().max()), 2.0 ** -23)
        print(f"speaker_similarity lens={'yes' if ln is not None else 'no'}: lib {got.tolist()}, fp64 {c64.tolist()}, bound {bound:.2e}")
        assert float((got - c64).abs().max()) <= bound
        assert float(c64.max() - c64.min()) > 10 * bound          # the pairs are told apart
    m = SpkSimWavLM("unused", 24000, model=enc)
    m.append(["a", "b", "c"], hyp.cuda(), ref.cuda())
    m.append(["d", "e", "f"], ref.cuda(), ref.cuda(), lens=lens.cuda())
    assert m.ids == list("abcdef") and len(m.scores) == 6
    assert all(abs(s - 1.0) < 1e-5 for s in m.scores[3:])
    want = speaker_similarity(hyp.cuda(), ref.cuda(), 24000, enc).cpu().tolist()
    assert m.scores[:3] == want
    s = m.summarize()
    assert s["max_id"] in "def" and s["min_id"] in "abc" and abs(s["average"] - sum(m.scores) / 6) < 1e-12
    # pool=False: the last hidden state instead of the x-vector (the reference's TTS speaker encoder), the same numbers as the stage
    from audiocodecs_amd import SpeakerEncoder

    emb, st = enc.forward(ref.cuda(), 24000, lens.cuda(), return_stages=True)
    last = SpeakerEncoder(state_dict=sd, arch=cfg, pool=False).forward(ref.cuda(), 24000, lens.cuda())
    assert last.shape == (B, st["hidden"].shape[2], cfg.hidden_size) and torch.equal(last, st["hidden"][-1])
    codec = Encodec(24000, num_codebooks=4, state_dict=checkpoint.synthetic_state_dict(TINY, seed=0), config=TINY).eval()
    sig = ref.cuda()
    a = codec.resynthesis_spk_sim(sig, enc)
    b = speaker_similarity(codec._resynthesize(sig, None)[1], sig, 24000, enc)
    assert torch.equal(a, b) and a.shape == (B,) and torch.isfinite(a).all()
