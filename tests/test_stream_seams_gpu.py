"""The five stream kernels (csrc/stream_path.hip: enc_stream, dec_stream, rb_stream6, rb_stream6m, rb_stream128m) against the fp64 CPU
oracle PER ELEMENT, at the batch sizes, lengths and developer switches where a clip is cut into segments (stream_seam_cases.py has the
geometry, the cases and the comparison; test_stream_seam_cases.py checks on the CPU that the cases reach every seam condition and that
the comparison sees what a seam bug would produce).

EnCodec: every module tap of sig_to_toks and of toks_to_sig (of the fp64 oracle's tokens), and the waveform as the last tap, with the
project's tap bar (5e-6 * max(1, amax) + 2e-5 * |ref|); tokens by the fp64-margin policy.  Switch-forced cases must also give the bits of
the default geometry.  Mimi: the folded kernels are invisible to the capture hook, so rb_stream6m<stem> and rb_stream128m<16> are judged
by sig_to_feats per element (bar derived from the fp32 Mimi oracle's own measured distance from the fp64 one, 1.10e-6 * max(1, amax), times
the factor 5.95 the EnCodec tap bar has over the EnCodec fp32 oracle: 6.61e-6 * max(1, amax) + 2e-5 * |ref|) plus tokens, and -- hook armed,
unfolded kernels -- by the taps of the first two residual blocks, so that a failure can be put down to the fold or not; rb_stream6m<head> by
the waveform per sample with the tap bar.

The geometry restated in stream_seam_cases.py can drift from stream_path.hip.  The comparison covers every element whatever the seams
are; the seam rows only say where the worst element sits.  The guards are the `profile_kernels` assertions and the bit equality of
switch-forced and default geometry."""
import numpy as np
import pytest
import torch

import parity_record
import stream_seam_cases as sc
from test_gpu_parity import capture
from test_oracle_golden import TAU

pytestmark = pytest.mark.gpu

STREAM = {"enc_stream_kernel", "dec_stream_kernel", "rb_stream6_kernel", "rb_stream128m_kernel"}


def base_names(codec, fn):
    return {s[0].split("<")[0] for s in codec.profile_kernels(fn)}


@pytest.fixture(scope="module")
def encodec(checkpoints):
    from audiocodecs_amd import Encodec

    cfg, sd = checkpoints("full", 0)
    codec = Encodec(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    codec.sig_to_toks(sc.noise(1, 1, 640).cuda())      # creates the native handle
    return codec


@pytest.fixture(scope="module")
def mimi(mimi_checkpoints):
    from audiocodecs_amd import Mimi

    cfg, sd = mimi_checkpoints("full", 0)
    codec = Mimi(24000, num_codebooks=8, state_dict=sd, config=cfg).eval()
    codec.sig_to_toks(sc.noise(1, 1, 1920).cuda())
    return codec


def split_taps(flat, names, shapes):
    """The capture buffer ([B][rows][C] per tap, in module order) as {tap: [B,C,rows]}."""
    out, off = {}, 0
    for tap in names:
        B, C, L = shapes[tap]
        out[tap] = flat[off : off + B * C * L].reshape(B, L, C).transpose(0, 2, 1)
        off += B * C * L
    assert off == flat.size, (off, flat.size)
    return out


def judge(case, taps, ref, failures, record, atol=sc.ATOL):
    for tap, r in ref.items():
        seams = sc.tap_seams(case, tap)
        w = sc.worst(taps[tap], r, seams, atol=atol)
        record[tap] = dict(err=w["err"], row=w["row"], seam_dist=w["seam_dist"], nseg=len(seams) + 1)
        print(f"{case['name']} {tap}: worst normalised error {w['err']:.3f} at clip {w['clip']} channel {w['channel']} row {w['row']} "
              f"(segment {w['segment']} of {len(seams) + 1}, {w['seam_dist']} rows from a seam)")
        if not w["err"] < 1.0:
            failures.append(f"{tap}: {w['err']:.3g} x the bar at clip {w['clip']}, channel {w['channel']}, row {w['row']}, "
                            f"segment {w['segment']} of {len(seams) + 1}, {w['seam_dist']} rows from the nearest seam (amax {w['amax']:.3g})")


@pytest.mark.parametrize("case", sc.ENCODEC_CASES, ids=lambda c: c["name"])
def test_encodec_taps_and_tokens_per_element_against_the_fp64_oracle(case, encodec):
    from audiocodecs_amd._native import debug_set

    codec = encodec
    inp = sc.case_input(case)
    ref = sc.encodec_reference(case)
    otoks = ref["toks"]
    dref = sc.encodec_decode_reference(otoks)
    nfloats = sc.capture_floats(case)
    knobs = case.get("knobs", {})
    failures, record = [], {}
    sig = inp["sig"].cuda() if "sig" in inp else None
    length = inp["length"].cuda() if "length" in inp else None
    gt = otoks.cuda()
    with torch.no_grad():
        default_enc = default_dec = None
        if knobs:      # the same input at the default geometry: the switch must not change one bit
            if sig is not None:
                _, default_enc = capture(codec, lambda: codec.sig_to_toks(sig, length), nfloats)
            default_wave, default_dec = capture(codec, lambda: codec.toks_to_sig(gt), nfloats)
        try:
            for k, v in knobs.items():
                debug_set(codec, k, v)
            if sig is not None:
                names = base_names(codec, lambda: codec.sig_to_toks(sig, length))
                if case["T"] >= sc.ENC_FUSED_MIN_T:
                    assert {"enc_stream_kernel", "rb_stream6_kernel", "rb_stream128m_kernel"} <= names, names
                    assert not ({"stem_kernel", "enc_front_kernel", "rb_fused6_kernel", "rb128_fused6_kernel"} & names), names
                else:      # below the fused front's threshold: the separate kernels, still against the oracle
                    assert "enc_stream_kernel" not in names and "enc_front_kernel" not in names and "stem_kernel" in names, names
                    assert {"rb_stream6_kernel", "rb_stream128m_kernel"} <= names, names
                toks, flat = capture(codec, lambda: codec.sig_to_toks(sig, length), nfloats)
                if default_enc is not None:
                    assert np.array_equal(flat, default_enc), "encoder taps depend on the segment switches"
                shapes = {t: ref["enc"][t].shape for t in sc.ENC_TAPS}
                judge(case, split_taps(flat, sc.ENC_TAPS, shapes), {t: ref["enc"][t] for t in sc.ENC_TAPS}, failures, record)
            names = base_names(codec, lambda: codec.toks_to_sig(gt))
            assert {"dec_stream_kernel", "rb_stream6_kernel", "rb_stream128m_kernel"} <= names, names
            assert not ({"head_kernel", "dec_tail_kernel", "rb_fused6_kernel", "rb128_fused6_kernel"} & names), names
            wave, flat = capture(codec, lambda: codec.toks_to_sig(gt), nfloats)
            if default_dec is not None:
                assert np.array_equal(flat, default_dec) and torch.equal(wave, default_wave), "decoder taps depend on the segment switches"
            shapes = {t: dref[t].shape for t in sc.DEC_TAPS}
            got = split_taps(flat, sc.DEC_TAPS, shapes)
            got["wave"] = wave.cpu().numpy()
            judge(case, got, dref, failures, record)
        finally:
            for k in knobs:
                debug_set(codec, k, sc.KNOB_DEFAULT[k])
    parity_record.record("encodec", "seam_" + case["name"], worst_norm_err_per_tap={t: r["err"] for t, r in record.items()},
                         worst_norm_err=max(r["err"] for r in record.values()), seam_taps=record,
                         waveform_rms_err=sc.rms(got["wave"] - dref["wave"]))
    if sig is not None:
        m64 = ref["margin"].numpy()
        mism, bad, excused = parity_record.tokens("encodec", "seam_" + case["name"], toks.cpu().numpy(), otoks.numpy(), m64, TAU)
        print(f"{case['name']}: {mism} of {m64.size} tokens differ, {bad} outside fp64 near-ties, {excused} excused")
        assert sc.excused_within_cap(m64, TAU)
        assert bad == 0 and mism <= excused, (mism, bad, excused)
    assert not failures, f"{case['name']}:\n  " + "\n  ".join(failures)


MIMI_TAPS = ["encoder.layers.0", "encoder.layers.1", "encoder.layers.3", "encoder.layers.4"]      # capture order: stem, block 64, conv, block 128


@pytest.mark.parametrize("case", sc.MIMI_ENC_CASES, ids=lambda c: c["name"])
def test_mimi_stem_fold_and_128_channel_block_against_the_fp64_oracle(case, mimi):
    codec = mimi
    sig = sc.mimi_case_input(case)["sig"].cuda()
    ref = sc.mimi_reference(case)
    with torch.no_grad():
        names = {s[0] for s in codec.profile_kernels(lambda: codec.sig_to_feats(sig))}
        assert "rb_stream6m_kernel<stem>" in names and "rb_stream128m_kernel<false>" in names and "stem_kernel" not in names, names
        feats = codec.sig_to_feats(sig).cpu().numpy()
        toks = codec.sig_to_toks(sig).cpu().numpy()
        _, flat = capture(codec, lambda: codec.sig_to_feats(sig), 1 << 27)      # hook armed: stem and block as separate kernels
    failures = []
    # unfolded kernels' taps (tap bar): a defect here is not the fold's
    record, off = {}, 0
    geo = sc.mimi_geometry(case)
    for tap in MIMI_TAPS:
        r = ref["taps"][tap]
        B, C, L = r.shape
        got = flat[off : off + r.size].reshape(B, L, C).transpose(0, 2, 1)
        off += r.size
        kern = {"encoder.layers.1": ("rb_stream6", case["T"]), "encoder.layers.4": geo["rb_stream128m"]}.get(tap)
        seams = sc.seam_rows(kern[0], case["B"], kern[1]) if kern else []
        w = sc.worst(got, r, seams)
        record[tap] = w["err"]
        print(f"{case['name']} {tap} (unfolded): worst normalised error {w['err']:.3f} at clip {w['clip']} row {w['row']}, {w['seam_dist']} rows from a seam")
        if not w["err"] < 1.0:
            failures.append(f"{tap} (separate kernels): {w['err']:.3g} x the bar at clip {w['clip']} row {w['row']}, {w['seam_dist']} rows from a seam")
    w = sc.worst(feats, ref["feats"], atol=sc.MIMI_FEATS_ATOL)
    print(f"{case['name']} feats: worst normalised error {w['err']:.3f} at clip {w['clip']} frame {w['channel']}")
    if not w["err"] < 1.0:
        failures.append(f"feats (folded kernels): {w['err']:.3g} x the bar at clip {w['clip']} frame {w['channel']} element {w['row']}")
    n, excused, per_clip = sc.near_tie_stats(ref["margin"], TAU)
    parity_record.record("mimi", "seam_" + case["name"], worst_norm_err_per_tap=record, feats_worst_norm_err=w["err"],
                         feats_atol=sc.MIMI_FEATS_ATOL, fp32_oracle_dev=sc.MIMI_FP32_DEV_FEATS, near_tie_share=excused / n)
    mism, bad, excused = parity_record.tokens("mimi", "seam_" + case["name"], toks, ref["toks"], ref["margin"], TAU)
    print(f"{case['name']}: {mism} of {n} tokens differ, {bad} outside fp64 near-ties, {excused} excused")
    assert bad == 0 and mism <= excused, (mism, bad, excused)
    assert not failures, f"{case['name']}:\n  " + "\n  ".join(failures)


@pytest.mark.parametrize("case", sc.MIMI_DEC_CASES, ids=lambda c: c["name"])
def test_mimi_head_fold_waveform_per_sample_against_the_fp64_oracle(case, mimi):
    codec = mimi
    toks = sc.mimi_case_input(case)["toks"].cuda()
    ref = sc.mimi_reference(case)["wave"]
    with torch.no_grad():
        names = {s[0] for s in codec.profile_kernels(lambda: codec.toks_to_sig(toks))}
        assert "rb_stream6m_kernel<head>" in names and "rb_fused6_head_kernel" not in names, names
        wave = codec.toks_to_sig(toks).cpu().numpy()
    seams = sc.seam_rows("rb_stream6m_head", case["B"], sc.MIMI_HOP * case["N"])
    w = sc.worst(wave, ref, seams)
    print(f"{case['name']} waveform: worst normalised error {w['err']:.3f} at clip {w['clip']} sample {w['row']} (segment {w['segment']} of "
          f"{len(seams) + 1}, {w['seam_dist']} rows from a seam)")
    parity_record.record("mimi", "seam_" + case["name"], worst_norm_err_per_tap={"wave": w["err"]}, worst_row=w["row"], seam_dist=w["seam_dist"],
                         waveform_rms_err=sc.rms(wave - ref))
    assert w["err"] < 1.0, w
