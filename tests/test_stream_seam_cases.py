"""What tests/test_stream_seams_gpu.py relies on, checked on the CPU: the restated segment geometry (stream_seam_cases.py) at hand-computed
points, that the case list reaches every seam condition for every stream kernel (conditions on the geometry, not measurements), that the
fp64 oracle's own near-ties stay inside the cap the token policy is allowed to excuse, and that the per-element comparison FAILS the
defects a seam bug would produce while the fp32 oracle PASSES against the fp64 one -- and that the whole-batch RMS bar misses such defects.

Oracle time of the whole seam module, measured on 16 CPU threads: EnCodec cases 9 s (fp64 tokens, margins, encoder and decoder taps of all
21 cases; 64 x 7000 alone 6.6 s), Mimi cases about 25 s (the 64-clip encode 13 s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stream_seam_cases as sc
from test_oracle_golden import TAU


def uses():
    """Every (kernel, case) launch of the case lists with its geometry inputs."""
    out = []
    for c in sc.ENCODEC_CASES:
        for tap in ("enc0", "enc4", "enc7", "dec7", "dec10", "wave"):
            g = sc.tap_geometry(c, tap)
            if g is not None:
                kern, rows, knob, waves, _ = g
                out.append(dict(kernel=kern, case=c["name"], B=c["B"], rows=rows, knob=knob, waves=waves, codec="encodec"))
    for c in sc.MIMI_ENC_CASES + sc.MIMI_DEC_CASES:
        for kern, (gk, rows) in sc.mimi_geometry(c).items():
            out.append(dict(kernel=gk, case=c["name"], B=c["B"], rows=rows, knob=0, waves=16, codec="mimi"))
    for u in out:
        u["unit"], u["seg"], u["nseg"] = sc.geometry(u["kernel"], u["B"], u["rows"], u["knob"], u["waves"])
        u["units"] = sc.cdiv(u["rows"], u["unit"])
        u["last_seg"] = u["units"] - (u["nseg"] - 1) * u["seg"]
        u["rem"] = u["rows"] % u["unit"]
    return out


USES = uses()


def of(kernel, codec=None):
    return [u for u in USES if u["kernel"] == kernel and (codec is None or u["codec"] == codec)]


def test_geometry_at_hand_computed_points():
    # stream_path.hip, by hand: 64 clips of 7000 samples
    assert sc.geometry("enc_stream", 64, 7000) == (32, 8, 28)                   # 219 chunks, max(8, cdiv(219, 64) = 4)
    assert sc.geometry("rb_stream6", 64, 3500) == (16, 4, 55)                   # 219 tiles over min(219, 64) segments
    assert sc.geometry("rb_stream128m", 64, 875, waves=12) == (16, 2, 28)       # 55 tiles, 3072 / 64 = 48 segments asked for
    assert sc.geometry("dec_stream", 64, 160 * 22) == (16, 8, 28)
    # a small batch: every tile its own segment; the switch makes them longer
    assert sc.geometry("rb_stream6", 3, 2401) == (16, 1, 151)
    assert sc.geometry("rb_stream6", 3, 2401, knob=4) == (16, 3, 51) and sc.last_segment_units("rb_stream6", 3, 2401, 4) == 1
    assert sc.geometry("rb_stream6", 3, 2401, knob=1000) == (16, 151, 1)
    assert sc.geometry("enc_stream", 20, 9600, knob=1000) == (32, 1000, 1)
    assert sc.geometry("rb_stream128m", 3, 875, waves=12) == (16, 1, 55)
    # Mimi: the stem block of 32 clips x 3840 samples, the head block's floor
    assert sc.geometry("rb_stream6m_stem", 32, 3840) == (16, 2, 120)
    assert sc.geometry("rb_stream6m_head", 3, 3840) == (16, 8, 30)
    assert sc.geometry("rb_stream6m_head", 64, 9600) == (16, 10, 60)
    assert sc.seam_rows("rb_stream6", 64, 3500)[:3] == [64, 128, 192] and sc.seam_rows("enc_stream", 64, 7000, scale=0.5)[0] == 128
    assert sc.seam_rows("dec_stream", 3, 160 * 16, knob=3, scale=2)[:2] == [96, 192]


def test_layer_map_row_counts_match_the_oracle():
    c = sc.encodec_case("b2_T503")
    ref = sc.encodec_reference(c, torch.float32)
    for tap, v in ref["enc"].items():
        assert v.shape[-1] == sc.tap_rows(tap, c["T"]), tap
    for tap, v in sc.encodec_decode_reference(ref["toks"], torch.float32).items():
        assert v.shape[-1] == sc.tap_rows(tap, c["T"]), tap
    assert sc.capture_floats(c) >= max(sum(v.size for v in ref["enc"].values()), 1)


@pytest.mark.parametrize("kernel", sc.KERNELS)
def test_every_kernel_is_segmented_by_the_batch_alone_and_by_its_switch(kernel):
    us = of(kernel)
    assert any(u["knob"] in (0, 1) and u["nseg"] >= 2 for u in us), "no batch-driven case with a seam"
    assert any(u["knob"] in (0, 1) and u["nseg"] >= 2 and u["seg"] >= 2 for u in us), "no batch-driven case with a multi-unit segment"
    if kernel in sc.KNOB:
        assert any(u["knob"] > 1 or (kernel != "rb_stream6" and u["knob"] > 0) for u in us if u["nseg"] >= 3), "no switch-forced case with nseg >= 3"
    else:
        assert any(u["nseg"] >= 3 for u in us)
    # the Mimi form of the 128-channel block (sixteen waves) has its own batch-driven multi-tile case
    if kernel == "rb_stream128m":
        assert any(u["nseg"] >= 2 and u["seg"] >= 2 for u in of(kernel, "mimi")) and any(u["nseg"] >= 2 and u["seg"] >= 2 for u in of(kernel, "encodec"))


@pytest.mark.parametrize("kernel", sc.KERNELS)
def test_last_segment_of_one_unit_and_of_full_length(kernel):
    us = of(kernel)
    assert any(u["seg"] >= 2 and u["nseg"] >= 2 and u["last_seg"] == 1 for u in us), "no short last segment of one unit"
    assert any(u["seg"] >= 2 and u["nseg"] >= 2 and u["last_seg"] == u["seg"] for u in us), "no case without a short segment"


@pytest.mark.parametrize("kernel", sc.KERNELS)
def test_last_tile_or_chunk_fill(kernel):
    """1, unit - 1, unit (full) and unit + 1 (= 1 row into the next) rows in the last tile or chunk -- or, for the kernels whose row count
    is a multiple of the unit whatever the frame count, the statement that a partial unit cannot occur."""
    us = of(kernel)
    if kernel in ("dec_stream", "rb_stream6m_head"):
        per_frame = 160 if kernel == "dec_stream" else sc.MIMI_HOP
        assert per_frame % sc.UNIT[kernel] == 0 and all(u["rem"] == 0 for u in us)
        return
    unit = sc.UNIT[kernel]
    rems = {u["rem"] for u in us}
    assert {1, unit - 1, 0} <= rems, rems
    assert any(u["rem"] == 1 and u["units"] >= 2 for u in us) and any(u["rem"] == 0 and u["units"] >= 2 for u in us)
    if kernel == "enc_stream":          # its output tile is 16 rows: also 15 / 16 / 17 samples into a chunk
        assert {15, 16, 17} <= rems, rems
    if kernel in ("rb_stream6", "rb_stream128m"):      # the decoder side never has a partial tile of 1 or 15 rows (40 N and 160 N rows)
        assert all(sc.tap_rows("dec7", N=n) % 8 == 0 and sc.tap_rows("dec10", N=n) % 16 == 0 for n in range(1, 64))


def test_rb_stream128m_row_tiles_modulo_four():
    assert {u["units"] % 4 for u in of("rb_stream128m", "encodec")} == {0, 1, 2, 3}


def test_enc_stream_lengths_around_a_chunk_boundary_and_the_fused_threshold():
    ts = {c["T"] for c in sc.ENCODEC_CASES if "T" in c}
    assert any({32 * k - 2, 32 * k - 1, 32 * k, 32 * k + 1, 32 * k + 2} <= ts for k in range(2, 400))
    assert sc.ENC_FUSED_MIN_T in ts and sc.ENC_FUSED_MIN_T - 1 in ts
    assert sc.tap_geometry(sc.encodec_case("b2_T63"), "enc0") is None and sc.tap_geometry(sc.encodec_case("b2_T64"), "enc0") is not None
    assert sc.tap_geometry(sc.encodec_case("b2_T63"), "enc4")[0] == "rb_stream6"      # only the fused front has the threshold


def test_head_floor_active_and_inactive():
    asked = [sc.cdiv(u["units"], min(u["units"], max(1, 4096 // u["B"]))) for u in of("rb_stream6m_head")]
    assert any(a < 8 for a in asked) and any(a > 8 for a in asked), asked


def test_ragged_mask_edge_falls_inside_a_warm_up_chunk():
    hits = 0
    for c in sc.ENCODEC_CASES:
        if "length" not in c:
            continue
        _, seg, nseg = sc.geometry("enc_stream", c["B"], c["T"], c.get("knobs", {}).get("front_seg", 0))
        for rel in c["length"]:
            e = sc.mask_edge(c["T"], rel)
            chunk = e // 32
            hits += e % 32 != 0 and (chunk + 1) % seg == 0 and (chunk + 1) // seg < nseg      # chunk is the one before a segment's first
        assert max(c["length"]) == 1.0
    assert hits >= 1


def test_knob_cases_name_real_switches_and_change_the_geometry():
    for c in sc.ENCODEC_CASES:
        for key in c.get("knobs", {}):
            assert key in sc.KNOB_DEFAULT
        if "knobs" in c:
            assert any(sc.tap_seams(c, t) != sc.tap_seams(c, t, default=True) for t in ("enc0", "enc4", "wave")), c["name"]


@pytest.mark.parametrize("case", [c for c in sc.ENCODEC_CASES if "T" in c], ids=lambda c: c["name"])
def test_fp64_near_ties_stay_inside_the_cap_encodec(case):
    m = sc.encodec_reference(case, taps=False)["margin"].numpy()
    n, excused, per_clip = sc.near_tie_stats(m, TAU)
    assert n == case["B"] * sc.frames(case["T"]) * 8
    assert sc.excused_within_cap(m, TAU), (n, excused, per_clip)


# Mimi's 2048-entry codebooks on noise put more frames near a tie than EnCodec's: the 64-clip case (the only way to segments of two tiles
# in the 128-channel block, which needs more than 4096 / B tiles) measures 6.9 to 10.6 % of its tokens in near-tie frames for every seed tried
# (31, 37 .. 40; the case uses 37: 106 of 1536).  The cap is NOT raised for it: the share is reported here and in the parity record, the test below marks the case as over
# the cap, and the GPU test therefore judges that case by its features per element, with the token policy as a second, weaker, check.
MIMI_OVER_CAP = {"mimi_b64_T4321"}


@pytest.mark.parametrize("case", sc.MIMI_ENC_CASES, ids=lambda c: c["name"])
def test_fp64_near_ties_stay_inside_the_cap_mimi(case):
    m = sc.mimi_reference(case)["margin"]
    n, excused, per_clip = sc.near_tie_stats(m, TAU)
    print(f"{case['name']}: {excused} of {n} tokens in fp64 near-tie frames ({100.0 * excused / n:.1f} %), at most {per_clip} such frames per clip")
    assert sc.excused_within_cap(m, TAU) == (case["name"] not in MIMI_OVER_CAP), (n, excused, per_clip)


def test_mimi_fp32_oracle_deviation_is_what_the_feature_bar_was_derived_from():
    """MIMI_FP32_DEV (relative to max(1, amax)) bounds the fp32 Mimi oracle's distance from the fp64 one per element, on features and on
    the waveform; the kernel's bar is that times the factor the EnCodec tap bar has over the EnCodec fp32 oracle."""
    devs = {}
    for case in sc.MIMI_ENC_CASES:
        a, b = sc.mimi_reference(case, torch.float32), sc.mimi_reference(case)
        devs[case["name"]] = sc.worst(a["feats"], b["feats"], atol=sc.MIMI_FP32_DEV_FEATS, rtol=0.0)["err"]
        assert sc.worst(a["feats"], b["feats"], atol=sc.MIMI_FEATS_ATOL, rtol=sc.RTOL)["err"] < 0.25
    assert 0.9 < max(devs.values()) <= 1.0, devs      # the constant is the measured maximum, neither below it nor padded
    assert abs(sc.MIMI_FEATS_ATOL - sc.MIMI_FP32_DEV_FEATS * sc.ATOL / sc.ENCODEC_FP32_DEV) < 1e-12


# ---- sensitivity: the defects a seam bug would produce, injected into the fp32 oracle's own taps

@pytest.fixture(scope="module")
def pair3():
    case = sc.encodec_case("b3_T4801_seg3")
    r64, r32 = sc.encodec_reference(case), sc.encodec_reference(case, torch.float32)
    d64 = sc.encodec_decode_reference(r64["toks"])
    d32 = sc.encodec_decode_reference(r64["toks"], torch.float32)
    return case, r64, r32, d64, d32


def test_the_fp32_oracle_passes_every_tap_against_the_fp64_oracle(pair3):
    case, r64, r32, d64, d32 = pair3
    worst = {}
    for tap in sc.ENC_TAPS:
        worst[tap] = sc.worst(r32["enc"][tap], r64["enc"][tap], sc.tap_seams(case, tap))["err"]
    for tap in sc.DEC_TAPS + ["wave"]:
        worst[tap] = sc.worst(d32[tap], d64[tap], sc.tap_seams(case, tap))["err"]
    assert max(worst.values()) < 0.5, worst          # the reference alone uses under half the bar


def rows_after_seam(x32, W, prefix, s, halo):
    """Rows s, s + 1 of a residual block's output when the k3 conv reads `halo` [B,C,2] in place of ELU(x) of rows s - 2, s - 1 (zeros: a
    segment that did not warm up its halo).  x32 [B,C,L] is the block's input."""
    xs = x32[:, :, s : s + 2]
    h = F.conv1d(torch.cat([halo, F.elu(xs)], -1), W[prefix + ".block.1.conv.weight"], W[prefix + ".block.1.conv.bias"])
    h = F.conv1d(F.elu(h), W[prefix + ".block.3.conv.weight"], W[prefix + ".block.3.conv.bias"])
    return F.conv1d(xs, W[prefix + ".shortcut.conv.weight"], W[prefix + ".shortcut.conv.bias"]) + h


def test_the_comparison_fails_seam_defects_the_rms_bar_does_not_see(pair3):
    from oracle import encodec_oracle as O

    case, r64, r32, d64, d32 = pair3
    _, W = sc._encodec_weights("float32")
    seen_by_rms = {}

    def check(name, tap, bad, ref, seams, expect_row):
        w = sc.worst(bad, ref, seams)
        assert w["err"] > 1.0, (name, w)
        assert w["row"] in expect_row, (name, w)
        seen_by_rms[name] = sc.rms(bad - ref) >= sc.RMS_BAR

    # (a) the two rows after a seam of enc4 (rb_stream6) computed from zero halo rows, in one clip
    seams = sc.tap_seams(case, "enc4")
    s = seams[len(seams) // 2]
    x = torch.from_numpy(r32["enc"]["enc3"][1:2])
    true_halo = F.elu(x[:, :, s - 2 : s])
    with torch.no_grad():
        same = rows_after_seam(x, W, "encoder.layers.4", s, true_halo).numpy()
        rows = rows_after_seam(x, W, "encoder.layers.4", s, torch.zeros_like(true_halo)).numpy()
        rows16 = rows_after_seam(x, W, "encoder.layers.4", s, true_halo.half().float()).numpy()
    assert np.abs(same[0] - r32["enc"]["enc4"][1, :, s : s + 2]).max() < 2e-6       # the injector itself reproduces the oracle's rows
    bad = r32["enc"]["enc4"].copy()
    bad[1, :, s : s + 2] = rows[0]
    check("zero halo", "enc4", bad, r64["enc"]["enc4"], seams, {s, s + 1})
    assert sc.worst(bad, r64["enc"]["enc4"], seams)["seam_dist"] <= 1 and sc.worst(bad, r64["enc"]["enc4"], seams)["clip"] == 1

    # (a') the same two rows from halo rows that lost their low half (the kernels carry the halo as two fp16 planes, split16.h)
    bad = r32["enc"]["enc4"].copy()
    bad[1, :, s : s + 2] = rows16[0]
    check("fp16 halo", "enc4", bad, r64["enc"]["enc4"], seams, {s, s + 1})

    # (b) one waveform sample duplicated from its neighbour at a seam of dec_stream
    seams = sc.tap_seams(case, "wave")
    s = seams[7]
    bad = d32["wave"].copy()
    bad[2, s] = bad[2, s - 1]
    check("duplicated row", "wave", bad, d64["wave"], seams, {s})

    # (c) the last row of the strided conv at odd T (enc3) with a zero in place of the reflected sample
    assert case["T"] % 2 == 1
    with torch.no_grad():
        xe = F.elu(torch.from_numpy(r32["enc"]["enc1"]))
        padded = F.pad(O.pad1d_reflect(xe, 2, 0), (0, 1))
        y = F.conv1d(padded, W["encoder.layers.3.conv.weight"], W["encoder.layers.3.conv.bias"], stride=2).numpy()
    bad = r32["enc"]["enc3"].copy()
    assert y.shape == bad.shape and np.abs(y[:, :, :-1] - bad[:, :, :-1]).max() < 1e-6
    bad[:, :, -1] = y[:, :, -1]
    check("zero for the reflected sample", "enc3", bad, r64["enc"]["enc3"], sc.tap_seams(case, "enc3"), {bad.shape[-1] - 1})

    # RMS over the whole batch against the 1e-5 bar (how the waveform is judged elsewhere): on these noise inputs the three gross defects
    # move a sample by 0.2 to 1.6, which even an RMS over 460 000 elements sees; the halo that lost its low half -- above the
    # per-element bar, as asserted above -- it does not
    assert seen_by_rms == {"zero halo": True, "fp16 halo": False, "duplicated row": True, "zero for the reflected sample": True}, seen_by_rms
