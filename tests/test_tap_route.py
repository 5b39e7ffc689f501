"""CPU check of the tap-GEMM routing (csrc/tap_route.h route_tap, through ac_debug_tap_route; no GPU): which kernel, tile
arrangement and epilogue every conv / linear layer of the four codecs gets.  Outputs are bit-identical whichever tap-GEMM
kernel runs, so the GPU tests cannot see a layer moving to another kernel; this table can.

The layer cases are the tap-GEMM launches of bench.py's default workloads (EnCodec / WavTokenizer 64 clips, Mimi 128, DAC 256;
10 s each) and of one 10 s clip, as run_tap saw them, plus those of the 16 kHz DAC model ("dac16": 64 clips and one clip of 10 s; its
stride-5 conv, K2560 J2 s5, and stride-5 transposed conv, N1920, are layers no other codec here has); each expected value is the profile record ac_profile_end reports for that
launch with the handle switch "prof_detail" on: the route's name and run_tap's shape suffix.  The switch cases come from the same
kind of runs with one developer switch set; the edge cases (exact products, misaligned operands, nine taps) follow run_tap's rules."""
import ctypes as C

import pytest

from test_native_abi import _built

ALIGNED, MISALIGNED = 1, 2      # pointer fields of the query: 0 = null


class Seg(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("x", "rel_len", "L", "cin", "s", "J", "dil", "pad", "lim", "kofs", "elu")] + \
               [("bs", C.c_int64), ("ts", C.c_int64)]


class Query(C.Structure):
    _fields_ = [(f, C.c_int32) for f in ("struct_size", "B", "M", "N", "Ktot", "nseg")] + [("seg", Seg * 2)] + \
               [(f, C.c_int32) for f in ("w", "y", "y_elu", "scale", "res", "alpha", "gelu", "tanh_out", "n_valid")] + \
               [(f, C.c_int64) for f in ("y_bs", "y_rs", "res_rs", "y_off", "y_len")] + \
               [(f, C.c_int32) for f in ("has_w6", "has_winv", "want_rowmode", "want_rows", "gemm_fp32",
                                         "tap_epi_staged", "tap_dil", "tap_pick", "tap8", "tap8_form", "tap8_spread")]


ROWMODE, DIRECT, REJECTED, SPREAD = 1, 2, 4, 8
SWITCH_DEFAULTS = dict(tap_epi_staged=0, tap_dil=1, tap_pick=-1, tap8=-1, tap8_form=0, tap8_spread=1)


def seg(L, cin, J=1, s=1, dil=1, pad=None, lim=None, kofs=0, bs=None, ts=None, x=ALIGNED, rel_len=0, elu=0):
    """One operand segment: a causal conv over [B][L][cin] channels-last rows unless told otherwise."""
    return dict(x=x, rel_len=rel_len, L=L, cin=cin, s=s, J=J, dil=dil, pad=(J - 1) * s if pad is None else pad,
                lim=L if lim is None else lim, kofs=kofs, elu=elu, bs=L * cin if bs is None else bs, ts=cin if ts is None else ts)


def layer(B, M, N, segs, **kw):
    """A tap-GEMM of the split16 product path: packed weights with their planes and scales, one output, no epilogue terms."""
    q = dict(B=B, M=M, N=N, Ktot=sum(g["J"] * g["s"] * g["cin"] for g in segs), segs=segs, w=ALIGNED, y=ALIGNED, y_elu=0,
             scale=0, res=0, alpha=0, gelu=0, tanh_out=0, n_valid=0, y_bs=M * N, y_rs=N, res_rs=0, y_off=0, y_len=0,
             has_w6=1, has_winv=1, want_rowmode=0, want_rows=0, gemm_fp32=0, **SWITCH_DEFAULTS)
    q.update(kw)
    return q


def route(q):
    """(name, flags) of route_tap for the query dict."""
    Q = Query()
    Q.struct_size = C.sizeof(Query)
    for k, v in q.items():
        if k != "segs":
            setattr(Q, k, v)
    Q.nseg = len(q["segs"])
    for i, g in enumerate(q["segs"]):
        for k, v in g.items():
            setattr(Q.seg[i], k, v)
    name = C.create_string_buffer(64)
    flags = C.c_int32(-1)
    assert _built().lib().ac_debug_tap_route(C.byref(Q), name, 64, C.byref(flags)) == 0
    return name.value.decode(), flags.value


def shape(q):
    """run_tap's prof_detail suffix of the launch (the tap_gemm4 / 6 / 8 records carry it)."""
    g = q["segs"][0]
    K = sum(s["J"] * s["s"] * s["cin"] for s in q["segs"])
    return f" B{q['B']} M{q['M']} N{q['N']} K{K} J{g['J']} s{g['s']}" + ("" if g["dil"] == 1 else " d3" if g["dil"] == 3 else " d9")


def record(q):
    """(profile record of the launch, flags): what ac_profile_end reports with "prof_detail" on."""
    name, flags = route(q)
    return (name if name.startswith("tap_gemm_kernel<") else name + shape(q)), flags


LAYERS = [
    # encodec B64
    ("encodec B64", layer(64, 30000, 128, [seg(120000, 64, J=2, s=4)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M30000 N128 K512 J2 s4", DIRECT),
    ("encodec B64", layer(64, 6000, 256, [seg(30000, 128, J=2, s=5)], y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT),
    ("encodec B64", layer(64, 6000, 128, [seg(6000, 256, J=3)], y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M6000 N128 K768 J3 s1", DIRECT),
    ("encodec B64", layer(64, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M6000 N256 K384 J1 s1", DIRECT),
    ("encodec B64", layer(64, 750, 512, [seg(6000, 256, J=2, s=8)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT | SPREAD),
    ("encodec B64", layer(64, 750, 128, [seg(750, 512, J=7)]), "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M750 N128 K3584 J7 s1", DIRECT),
    ("encodec B64", layer(64, 750, 512, [seg(750, 128, J=7)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K896 J7 s1", DIRECT | SPREAD),
    ("encodec B64", layer(64, 750, 2048, [seg(750, 512, J=2)], y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M750 N2048 K1024 J2 s1", DIRECT),
    ("encodec B64", layer(64, 6000, 640, [seg(6000, 256, J=2)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M6000 N640 K512 J2 s1", DIRECT),
    ("encodec B64", layer(64, 30000, 256, [seg(30000, 128, J=2)]), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M30000 N256 K256 J2 s1", DIRECT),
    # mimi B128
    ("mimi B128", layer(128, 60000, 128, [seg(240000, 64, J=2, s=4)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B128 M60000 N128 K512 J2 s4", DIRECT),
    ("mimi B128", layer(128, 12000, 256, [seg(60000, 128, J=2, s=5)], y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M12000 N256 K1280 J2 s5", DIRECT),
    ("mimi B128", layer(128, 12000, 128, [seg(12000, 256, J=3)], y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B128 M12000 N128 K768 J3 s1", DIRECT),
    ("mimi B128", layer(128, 12000, 256, [seg(12000, 128)], res=1, res_rs=256, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M12000 N256 K128 J1 s1", 0),
    ("mimi B128", layer(128, 2000, 512, [seg(12000, 256, J=2, s=6)], y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M2000 N512 K3072 J2 s6", DIRECT),
    ("mimi B128", layer(128, 2000, 256, [seg(2000, 512, J=3)], y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M2000 N256 K1536 J3 s1", DIRECT),
    ("mimi B128", layer(128, 2000, 512, [seg(2000, 256)], res=1, res_rs=512, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M2000 N512 K256 J1 s1", 0),
    ("mimi B128", layer(128, 250, 1024, [seg(2000, 512, J=2, s=8)], y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M250 N1024 K8192 J2 s8", DIRECT),
    ("mimi B128", layer(128, 250, 512, [seg(250, 1024, J=3)]), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M250 N512 K3072 J3 s1", DIRECT),
    ("mimi B128", layer(1, 32000, 1536, [seg(32000, 512, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M32000 N1536 K512 J1 s1", ROWMODE),
    ("mimi B128", layer(1, 32000, 512, [seg(32000, 512, bs=0)], res=1, res_rs=512, scale=1, want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M32000 N512 K512 J1 s1", ROWMODE),
    ("mimi B128", layer(1, 32000, 2048, [seg(32000, 512, bs=0)], gelu=1, want_rowmode=1, want_rows=1, y_bs=0), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M32000 N2048 K512 J1 s1", ROWMODE),
    ("mimi B128", layer(1, 32000, 512, [seg(32000, 2048, bs=0)], res=1, res_rs=512, scale=1, want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M32000 N512 K2048 J1 s1", ROWMODE),
    ("mimi B128", layer(128, 125, 512, [seg(250, 512, J=2, s=2)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B128 M125 N512 K2048 J2 s2", DIRECT | SPREAD),
    ("mimi B128", layer(1, 16000, 512, [seg(16000, 512, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M16000 N512 K512 J1 s1", ROWMODE | SPREAD),
    ("mimi B128", layer(1, 16000, 512, [seg(16000, 512, bs=0)], has_w6=0, has_winv=0, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M16000 N512 K512 J1 s1", 0),
    ("mimi B128", layer(128, 250, 1024, [seg(250, 512, J=7)], y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M250 N1024 K3584 J7 s1", DIRECT),
    ("mimi B128", layer(128, 250, 4096, [seg(250, 1024, J=2)], y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M250 N4096 K2048 J2 s1", DIRECT),
    ("mimi B128", layer(128, 2000, 1536, [seg(2000, 512, J=2)], y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M2000 N1536 K1024 J2 s1", DIRECT),
    ("mimi B128", layer(128, 12000, 640, [seg(12000, 256, J=2)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B128 M12000 N640 K512 J2 s1", DIRECT),
    ("mimi B128", layer(128, 60000, 256, [seg(60000, 128, J=2)]), "tap_gemm8_kernel<2, 4, 4, 2, 2> B128 M60000 N256 K256 J2 s1", DIRECT),
    # dac B256
    ("dac B256", layer(63, 441000, 64, [seg(441000, 64, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B63 M441000 N64 K448 J7 s1", DIRECT),
    ("dac B256", layer(63, 441000, 64, [seg(441000, 64)], alpha=1, res=1, res_rs=64, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B63 M441000 N64 K64 J1 s1", DIRECT),
    ("dac B256", layer(63, 441000, 64, [seg(441000, 64, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B63 M441000 N64 K448 J7 s1 d3", DIRECT),
    ("dac B256", layer(63, 441000, 64, [seg(441000, 64, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B63 M441000 N64 K448 J7 s1 d9", DIRECT),
    ("dac B256", layer(63, 220500, 128, [seg(441000, 64, J=2, pad=1, s=2)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B63 M220500 N128 K256 J2 s2", 0),
    ("dac B256", layer(63, 220500, 128, [seg(220500, 128, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B63 M220500 N128 K896 J7 s1", 0),
    ("dac B256", layer(63, 220500, 128, [seg(220500, 128)], alpha=1, res=1, res_rs=128, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B63 M220500 N128 K128 J1 s1", 0),
    ("dac B256", layer(63, 220500, 128, [seg(220500, 128, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B63 M220500 N128 K896 J7 s1 d3", 0),
    ("dac B256", layer(63, 220500, 128, [seg(220500, 128, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B63 M220500 N128 K896 J7 s1 d9", 0),
    ("dac B256", layer(63, 55125, 256, [seg(220500, 128, J=2, pad=2, s=4)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B63 M55125 N256 K1024 J2 s4", 0),
    ("dac B256", layer(63, 55125, 256, [seg(55125, 256, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B63 M55125 N256 K1792 J7 s1", 0),
    ("dac B256", layer(63, 55125, 256, [seg(55125, 256)], alpha=1, res=1, res_rs=256, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B63 M55125 N256 K256 J1 s1", 0),
    ("dac B256", layer(63, 55125, 256, [seg(55125, 256, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B63 M55125 N256 K1792 J7 s1 d3", 0),
    ("dac B256", layer(63, 55125, 256, [seg(55125, 256, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B63 M55125 N256 K1792 J7 s1 d9", 0),
    ("dac B256", layer(63, 6890, 512, [seg(55125, 256, J=2, pad=4, s=8)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B63 M6890 N512 K4096 J2 s8", 0),
    ("dac B256", layer(63, 6890, 512, [seg(6890, 512, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B63 M6890 N512 K3584 J7 s1", 0),
    ("dac B256", layer(63, 6890, 512, [seg(6890, 512)], alpha=1, res=1, res_rs=512, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B63 M6890 N512 K512 J1 s1", 0),
    ("dac B256", layer(63, 6890, 512, [seg(6890, 512, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B63 M6890 N512 K3584 J7 s1 d3", 0),
    ("dac B256", layer(63, 6890, 512, [seg(6890, 512, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B63 M6890 N512 K3584 J7 s1 d9", 0),
    ("dac B256", layer(63, 861, 1024, [seg(6890, 512, J=2, pad=4, s=8)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B63 M861 N1024 K8192 J2 s8", SPREAD),
    ("dac B256", layer(63, 861, 1024, [seg(861, 1024, J=3, pad=1)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B63 M861 N1024 K3072 J3 s1", DIRECT | SPREAD),
    ("dac B256", layer(4, 441000, 64, [seg(441000, 64, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B4 M441000 N64 K448 J7 s1", DIRECT),
    ("dac B256", layer(4, 441000, 64, [seg(441000, 64)], alpha=1, res=1, res_rs=64, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B4 M441000 N64 K64 J1 s1", DIRECT),
    ("dac B256", layer(4, 441000, 64, [seg(441000, 64, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B4 M441000 N64 K448 J7 s1 d3", DIRECT),
    ("dac B256", layer(4, 441000, 64, [seg(441000, 64, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B4 M441000 N64 K448 J7 s1 d9", DIRECT),
    ("dac B256", layer(4, 220500, 128, [seg(441000, 64, J=2, pad=1, s=2)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M220500 N128 K256 J2 s2", 0),
    ("dac B256", layer(4, 220500, 128, [seg(220500, 128, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M220500 N128 K896 J7 s1", 0),
    ("dac B256", layer(4, 220500, 128, [seg(220500, 128)], alpha=1, res=1, res_rs=128, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M220500 N128 K128 J1 s1", 0),
    ("dac B256", layer(4, 220500, 128, [seg(220500, 128, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M220500 N128 K896 J7 s1 d3", 0),
    ("dac B256", layer(4, 220500, 128, [seg(220500, 128, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M220500 N128 K896 J7 s1 d9", 0),
    ("dac B256", layer(4, 55125, 256, [seg(220500, 128, J=2, pad=2, s=4)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B4 M55125 N256 K1024 J2 s4", SPREAD),
    ("dac B256", layer(4, 55125, 256, [seg(55125, 256, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B4 M55125 N256 K1792 J7 s1", SPREAD),
    ("dac B256", layer(4, 55125, 256, [seg(55125, 256)], alpha=1, res=1, res_rs=256, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B4 M55125 N256 K256 J1 s1", SPREAD),
    ("dac B256", layer(4, 55125, 256, [seg(55125, 256, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M55125 N256 K1792 J7 s1 d3", 0),
    ("dac B256", layer(4, 55125, 256, [seg(55125, 256, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M55125 N256 K1792 J7 s1 d9", 0),
    ("dac B256", layer(4, 6890, 512, [seg(55125, 256, J=2, pad=4, s=8)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B4 M6890 N512 K4096 J2 s8", 0),
    ("dac B256", layer(4, 6890, 512, [seg(6890, 512, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B4 M6890 N512 K3584 J7 s1", 0),
    ("dac B256", layer(4, 6890, 512, [seg(6890, 512)], alpha=1, res=1, res_rs=512, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B4 M6890 N512 K512 J1 s1", 0),
    ("dac B256", layer(4, 6890, 512, [seg(6890, 512, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B4 M6890 N512 K3584 J7 s1 d3", 0),
    ("dac B256", layer(4, 6890, 512, [seg(6890, 512, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B4 M6890 N512 K3584 J7 s1 d9", 0),
    ("dac B256", layer(4, 861, 1024, [seg(6890, 512, J=2, pad=4, s=8)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B4 M861 N1024 K8192 J2 s8", 0),
    ("dac B256", layer(4, 861, 1024, [seg(861, 1024, J=3, pad=1)]), "tap_gemm6_kernel<1, 8, 4, 1, 2> B4 M861 N1024 K3072 J3 s1", DIRECT),
    ("dac B256", layer(42, 861, 1536, [seg(861, 1024, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B42 M861 N1536 K7168 J7 s1", SPREAD),
    ("dac B256", layer(42, 862, 6144, [seg(861, 1536, J=2)], alpha=1, y_bs=5289984, y_elu=1, y_len=5289984, y_off=-3072), "tap_gemm8_kernel<2, 4, 2, 2, 2> B42 M862 N6144 K3072 J2 s1", SPREAD),
    ("dac B256", layer(42, 6888, 768, [seg(6888, 768, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B42 M6888 N768 K5376 J7 s1", 0),
    ("dac B256", layer(42, 6888, 768, [seg(6888, 768)], alpha=1, res=1, res_rs=768, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B42 M6888 N768 K768 J1 s1", 0),
    ("dac B256", layer(42, 6888, 768, [seg(6888, 768, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B42 M6888 N768 K5376 J7 s1 d3", 0),
    ("dac B256", layer(42, 6888, 768, [seg(6888, 768, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B42 M6888 N768 K5376 J7 s1 d9", 0),
    ("dac B256", layer(42, 6889, 3072, [seg(6888, 768, J=2)], alpha=1, y_bs=21159936, y_elu=1, y_len=21159936, y_off=-1536), "tap_gemm8_kernel<2, 4, 4, 2, 2> B42 M6889 N3072 K1536 J2 s1", 0),
    ("dac B256", layer(42, 55104, 384, [seg(55104, 384, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B42 M55104 N384 K2688 J7 s1", 0),
    ("dac B256", layer(42, 55104, 384, [seg(55104, 384)], alpha=1, res=1, res_rs=384, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B42 M55104 N384 K384 J1 s1", 0),
    ("dac B256", layer(42, 55104, 384, [seg(55104, 384, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B42 M55104 N384 K2688 J7 s1 d3", 0),
    ("dac B256", layer(42, 55104, 384, [seg(55104, 384, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B42 M55104 N384 K2688 J7 s1 d9", 0),
    ("dac B256", layer(42, 55105, 768, [seg(55104, 384, J=2)], alpha=1, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-384), "tap_gemm8_kernel<2, 4, 4, 2, 2> B42 M55105 N768 K768 J2 s1", 0),
    ("dac B256", layer(42, 220416, 192, [seg(220416, 192, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B42 M220416 N192 K1344 J7 s1", 0),
    ("dac B256", layer(42, 220416, 192, [seg(220416, 192)], alpha=1, res=1, res_rs=192, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B42 M220416 N192 K192 J1 s1", 0),
    ("dac B256", layer(42, 220416, 192, [seg(220416, 192, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B42 M220416 N192 K1344 J7 s1 d3", 0),
    ("dac B256", layer(42, 220416, 192, [seg(220416, 192, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B42 M220416 N192 K1344 J7 s1 d9", 0),
    ("dac B256", layer(42, 220417, 192, [seg(220416, 192, J=2)], alpha=1, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-96), "tap_gemm6_kernel<2, 2, 2, 3, 2> B42 M220417 N192 K384 J2 s1", 0),
    ("dac B256", layer(4, 861, 1536, [seg(861, 1024, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B4 M861 N1536 K7168 J7 s1", 0),
    ("dac B256", layer(4, 862, 6144, [seg(861, 1536, J=2)], alpha=1, y_bs=5289984, y_elu=1, y_len=5289984, y_off=-3072), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M862 N6144 K3072 J2 s1", 0),
    ("dac B256", layer(4, 6888, 768, [seg(6888, 768, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M6888 N768 K5376 J7 s1", 0),
    ("dac B256", layer(4, 6888, 768, [seg(6888, 768)], alpha=1, res=1, res_rs=768, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M6888 N768 K768 J1 s1", 0),
    ("dac B256", layer(4, 6888, 768, [seg(6888, 768, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B4 M6888 N768 K5376 J7 s1 d3", 0),
    ("dac B256", layer(4, 6888, 768, [seg(6888, 768, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B4 M6888 N768 K5376 J7 s1 d9", 0),
    ("dac B256", layer(4, 6889, 3072, [seg(6888, 768, J=2)], alpha=1, y_bs=21159936, y_elu=1, y_len=21159936, y_off=-1536), "tap_gemm8_kernel<2, 4, 4, 2, 2> B4 M6889 N3072 K1536 J2 s1", 0),
    ("dac B256", layer(4, 55104, 384, [seg(55104, 384, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M55104 N384 K2688 J7 s1", 0),
    ("dac B256", layer(4, 55104, 384, [seg(55104, 384)], alpha=1, res=1, res_rs=384, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B4 M55104 N384 K384 J1 s1", 0),
    ("dac B256", layer(4, 55104, 384, [seg(55104, 384, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B4 M55104 N384 K2688 J7 s1 d3", 0),
    ("dac B256", layer(4, 55104, 384, [seg(55104, 384, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B4 M55104 N384 K2688 J7 s1 d9", 0),
    ("dac B256", layer(4, 55105, 768, [seg(55104, 384, J=2)], alpha=1, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-384), "tap_gemm8_kernel<2, 4, 4, 2, 2> B4 M55105 N768 K768 J2 s1", 0),
    ("dac B256", layer(4, 220416, 192, [seg(220416, 192, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B4 M220416 N192 K1344 J7 s1", 0),
    ("dac B256", layer(4, 220416, 192, [seg(220416, 192)], alpha=1, res=1, res_rs=192, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B4 M220416 N192 K192 J1 s1", 0),
    ("dac B256", layer(4, 220416, 192, [seg(220416, 192, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B4 M220416 N192 K1344 J7 s1 d3", 0),
    ("dac B256", layer(4, 220416, 192, [seg(220416, 192, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B4 M220416 N192 K1344 J7 s1 d9", 0),
    ("dac B256", layer(4, 220417, 192, [seg(220416, 192, J=2)], alpha=1, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-96), "tap_gemm6_kernel<2, 2, 2, 3, 2> B4 M220417 N192 K384 J2 s1", 0),
    # wavtokenizer B64
    ("wavtokenizer B64", layer(64, 60000, 64, [seg(240000, 32, J=2, lim=240002, pad=2, s=4)]), "tap_gemm6_kernel<2, 2, 2, 1, 2> B64 M60000 N64 K256 J2 s4", 0),
    ("wavtokenizer B64", layer(64, 12000, 128, [seg(60000, 64, J=2, lim=60002, pad=3, s=5)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M12000 N128 K640 J2 s5", DIRECT),
    ("wavtokenizer B64", layer(64, 2400, 256, [seg(12000, 128, J=2, lim=12002, pad=3, s=5)], y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M2400 N256 K1280 J2 s5", DIRECT | SPREAD),
    ("wavtokenizer B64", layer(64, 2400, 128, [seg(2400, 256, J=3, lim=2401, pad=1)], y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M2400 N128 K768 J3 s1", DIRECT),
    ("wavtokenizer B64", layer(64, 2400, 256, [seg(2400, 128), seg(2400, 256, kofs=128)], y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M2400 N256 K384 J1 s1", DIRECT),
    ("wavtokenizer B64", layer(64, 400, 512, [seg(2400, 256, J=2, lim=2403, pad=3, s=6)]), "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M400 N512 K3072 J2 s6", DIRECT),
    ("wavtokenizer B64", layer(64, 400, 512, [seg(400, 512, J=7, lim=403, pad=3)]), "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M400 N512 K3584 J7 s1", DIRECT),
    ("wavtokenizer B64", layer(64, 400, 768, [seg(400, 512, J=7, pad=3)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M400 N768 K3584 J7 s1", DIRECT),
    ("wavtokenizer B64", layer(64, 400, 768, [seg(400, 768, J=3, pad=1)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M400 N768 K2304 J3 s1", DIRECT),
    ("wavtokenizer B64", layer(64, 400, 768, [seg(400, 768, J=3, pad=1)], res=1, res_rs=768), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M400 N768 K2304 J3 s1", 0),
    ("wavtokenizer B64", layer(1, 25600, 2304, [seg(25600, 768, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M25600 N2304 K768 J1 s1", ROWMODE),
    ("wavtokenizer B64", layer(1, 25600, 768, [seg(25600, 768, bs=0)], res=1, res_rs=768, want_rowmode=1, y_bs=0), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M25600 N768 K768 J1 s1", ROWMODE),
    ("wavtokenizer B64", layer(1, 25600, 768, [seg(25600, 2304, bs=0)], res=1, res_rs=768, scale=1, want_rowmode=1, y_bs=0), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M25600 N768 K2304 J1 s1", ROWMODE),
    ("wavtokenizer B64", layer(1, 25600, 2432, [seg(25600, 768, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M25600 N2432 K768 J1 s1", ROWMODE),
    ("wavtokenizer B64", layer(64, 403, 640, [seg(400, 2432, J=4)], n_valid=600, y_bs=240000, y_len=240000, y_off=-900, y_rs=600), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M403 N640 K9728 J4 s1", 0),
    # encodec B1
    ("encodec B1", layer(1, 30000, 128, [seg(120000, 64, J=2, s=4)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M30000 N128 K512 J2 s4", DIRECT),
    ("encodec B1", layer(1, 6000, 256, [seg(30000, 128, J=2, s=5)], y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6000 N256 K1280 J2 s5", DIRECT),
    ("encodec B1", layer(1, 6000, 128, [seg(6000, 256, J=3)], y=0, y_elu=1), "tap_gemm8_kernel<4, 2, 2, 2, 2> B1 M6000 N128 K768 J3 s1", DIRECT),
    ("encodec B1", layer(1, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6000 N256 K384 J1 s1", DIRECT),
    ("encodec B1", layer(1, 750, 512, [seg(6000, 256, J=2, s=8)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M750 N512 K4096 J2 s8", DIRECT | SPREAD),
    ("encodec B1", layer(1, 750, 128, [seg(750, 512, J=7)]), "tap_gemm8_kernel<4, 2, 2, 2, 2> B1 M750 N128 K3584 J7 s1", DIRECT),
    ("encodec B1", layer(1, 750, 512, [seg(750, 128, J=7)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M750 N512 K896 J7 s1", DIRECT | SPREAD),
    ("encodec B1", layer(1, 750, 2048, [seg(750, 512, J=2)], y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M750 N2048 K1024 J2 s1", DIRECT),
    ("encodec B1", layer(1, 6000, 640, [seg(6000, 256, J=2)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M6000 N640 K512 J2 s1", DIRECT),
    ("encodec B1", layer(1, 30000, 256, [seg(30000, 128, J=2)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M30000 N256 K256 J2 s1", DIRECT | SPREAD),
    # mimi B1
    ("mimi B1", layer(1, 60000, 128, [seg(240000, 64, J=2, s=4)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M60000 N128 K512 J2 s4", DIRECT),
    ("mimi B1", layer(1, 12000, 256, [seg(60000, 128, J=2, s=5)], y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M12000 N256 K1280 J2 s5", DIRECT),
    ("mimi B1", layer(1, 12000, 128, [seg(12000, 256, J=3)], y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M12000 N128 K768 J3 s1", DIRECT),
    ("mimi B1", layer(1, 12000, 256, [seg(12000, 128)], res=1, res_rs=256, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M12000 N256 K128 J1 s1", 0),
    ("mimi B1", layer(1, 2000, 512, [seg(12000, 256, J=2, s=6)], y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N512 K3072 J2 s6", DIRECT | SPREAD),
    ("mimi B1", layer(1, 2000, 256, [seg(2000, 512, J=3)], y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N256 K1536 J3 s1", DIRECT | SPREAD),
    ("mimi B1", layer(1, 2000, 512, [seg(2000, 256)], res=1, res_rs=512, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N512 K256 J1 s1", SPREAD),
    ("mimi B1", layer(1, 250, 1024, [seg(2000, 512, J=2, s=8)], y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N1024 K8192 J2 s8", DIRECT | SPREAD),
    ("mimi B1", layer(1, 250, 512, [seg(250, 1024, J=3)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N512 K3072 J3 s1", DIRECT | SPREAD),
    ("mimi B1", layer(1, 250, 1536, [seg(250, 512, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N1536 K512 J1 s1", ROWMODE | SPREAD),
    ("mimi B1", layer(1, 250, 512, [seg(250, 512, bs=0)], res=1, res_rs=512, scale=1, want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N512 K512 J1 s1", ROWMODE | SPREAD),
    ("mimi B1", layer(1, 250, 2048, [seg(250, 512, bs=0)], gelu=1, want_rowmode=1, want_rows=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N2048 K512 J1 s1", ROWMODE | SPREAD),
    ("mimi B1", layer(1, 250, 512, [seg(250, 2048, bs=0)], res=1, res_rs=512, scale=1, want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N512 K2048 J1 s1", ROWMODE | SPREAD),
    ("mimi B1", layer(1, 125, 512, [seg(250, 512, J=2, s=2)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M125 N512 K2048 J2 s2", DIRECT | SPREAD),
    ("mimi B1", layer(1, 125, 512, [seg(125, 512, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M125 N512 K512 J1 s1", ROWMODE | SPREAD),
    ("mimi B1", layer(1, 125, 512, [seg(125, 512, bs=0)], has_w6=0, has_winv=0, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M125 N512 K512 J1 s1", 0),
    ("mimi B1", layer(1, 250, 1024, [seg(250, 512, J=7)], y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N1024 K3584 J7 s1", DIRECT | SPREAD),
    ("mimi B1", layer(1, 250, 4096, [seg(250, 1024, J=2)], y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N4096 K2048 J2 s1", DIRECT | SPREAD),
    ("mimi B1", layer(1, 2000, 1536, [seg(2000, 512, J=2)], y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M2000 N1536 K1024 J2 s1", DIRECT),
    ("mimi B1", layer(1, 12000, 640, [seg(12000, 256, J=2)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M12000 N640 K512 J2 s1", DIRECT),
    ("mimi B1", layer(1, 60000, 256, [seg(60000, 128, J=2)]), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M60000 N256 K256 J2 s1", DIRECT),
    # dac B1
    ("dac B1", layer(1, 441000, 64, [seg(441000, 64, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M441000 N64 K448 J7 s1", DIRECT),
    ("dac B1", layer(1, 441000, 64, [seg(441000, 64)], alpha=1, res=1, res_rs=64, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M441000 N64 K64 J1 s1", DIRECT),
    ("dac B1", layer(1, 441000, 64, [seg(441000, 64, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M441000 N64 K448 J7 s1 d3", DIRECT),
    ("dac B1", layer(1, 441000, 64, [seg(441000, 64, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M441000 N64 K448 J7 s1 d9", DIRECT),
    ("dac B1", layer(1, 220500, 128, [seg(441000, 64, J=2, pad=1, s=2)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M220500 N128 K256 J2 s2", 0),
    ("dac B1", layer(1, 220500, 128, [seg(220500, 128, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M220500 N128 K896 J7 s1", 0),
    ("dac B1", layer(1, 220500, 128, [seg(220500, 128)], alpha=1, res=1, res_rs=128, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M220500 N128 K128 J1 s1", 0),
    ("dac B1", layer(1, 220500, 128, [seg(220500, 128, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M220500 N128 K896 J7 s1 d3", 0),
    ("dac B1", layer(1, 220500, 128, [seg(220500, 128, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M220500 N128 K896 J7 s1 d9", 0),
    ("dac B1", layer(1, 55125, 256, [seg(220500, 128, J=2, pad=2, s=4)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55125 N256 K1024 J2 s4", 0),
    ("dac B1", layer(1, 55125, 256, [seg(55125, 256, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55125 N256 K1792 J7 s1", 0),
    ("dac B1", layer(1, 55125, 256, [seg(55125, 256)], alpha=1, res=1, res_rs=256, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55125 N256 K256 J1 s1", 0),
    ("dac B1", layer(1, 55125, 256, [seg(55125, 256, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B1 M55125 N256 K1792 J7 s1 d3", 0),
    ("dac B1", layer(1, 55125, 256, [seg(55125, 256, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B1 M55125 N256 K1792 J7 s1 d9", 0),
    ("dac B1", layer(1, 6890, 512, [seg(55125, 256, J=2, pad=4, s=8)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6890 N512 K4096 J2 s8", 0),
    ("dac B1", layer(1, 6890, 512, [seg(6890, 512, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6890 N512 K3584 J7 s1", 0),
    ("dac B1", layer(1, 6890, 512, [seg(6890, 512)], alpha=1, res=1, res_rs=512, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6890 N512 K512 J1 s1", 0),
    ("dac B1", layer(1, 6890, 512, [seg(6890, 512, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6890 N512 K3584 J7 s1 d3", 0),
    ("dac B1", layer(1, 6890, 512, [seg(6890, 512, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6890 N512 K3584 J7 s1 d9", 0),
    ("dac B1", layer(1, 861, 1024, [seg(6890, 512, J=2, pad=4, s=8)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M861 N1024 K8192 J2 s8", SPREAD),
    ("dac B1", layer(1, 861, 1024, [seg(861, 1024, J=3, pad=1)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M861 N1024 K3072 J3 s1", DIRECT | SPREAD),
    ("dac B1", layer(1, 861, 1536, [seg(861, 1024, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M861 N1536 K7168 J7 s1", 0),
    ("dac B1", layer(1, 862, 6144, [seg(861, 1536, J=2)], alpha=1, y_bs=5289984, y_elu=1, y_len=5289984, y_off=-3072), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M862 N6144 K3072 J2 s1", 0),
    ("dac B1", layer(1, 6888, 768, [seg(6888, 768, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6888 N768 K5376 J7 s1", 0),
    ("dac B1", layer(1, 6888, 768, [seg(6888, 768)], alpha=1, res=1, res_rs=768, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6888 N768 K768 J1 s1", 0),
    ("dac B1", layer(1, 6888, 768, [seg(6888, 768, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6888 N768 K5376 J7 s1 d3", 0),
    ("dac B1", layer(1, 6888, 768, [seg(6888, 768, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6888 N768 K5376 J7 s1 d9", 0),
    ("dac B1", layer(1, 6889, 3072, [seg(6888, 768, J=2)], alpha=1, y_bs=21159936, y_elu=1, y_len=21159936, y_off=-1536), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M6889 N3072 K1536 J2 s1", 0),
    ("dac B1", layer(1, 55104, 384, [seg(55104, 384, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M55104 N384 K2688 J7 s1", 0),
    ("dac B1", layer(1, 55104, 384, [seg(55104, 384)], alpha=1, res=1, res_rs=384, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M55104 N384 K384 J1 s1", 0),
    ("dac B1", layer(1, 55104, 384, [seg(55104, 384, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B1 M55104 N384 K2688 J7 s1 d3", 0),
    ("dac B1", layer(1, 55104, 384, [seg(55104, 384, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B1 M55104 N384 K2688 J7 s1 d9", 0),
    ("dac B1", layer(1, 55105, 768, [seg(55104, 384, J=2)], alpha=1, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-384), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55105 N768 K768 J2 s1", 0),
    ("dac B1", layer(1, 220416, 192, [seg(220416, 192, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M220416 N192 K1344 J7 s1", 0),
    ("dac B1", layer(1, 220416, 192, [seg(220416, 192)], alpha=1, res=1, res_rs=192, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M220416 N192 K192 J1 s1", 0),
    ("dac B1", layer(1, 220416, 192, [seg(220416, 192, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B1 M220416 N192 K1344 J7 s1 d3", 0),
    ("dac B1", layer(1, 220416, 192, [seg(220416, 192, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B1 M220416 N192 K1344 J7 s1 d9", 0),
    ("dac B1", layer(1, 220417, 192, [seg(220416, 192, J=2)], alpha=1, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-96), "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M220417 N192 K384 J2 s1", 0),
    # dac16 B64 (config.DAC_16KHZ, strides (2,4,5,8), 64 clips x 10 s)
    ("dac16 B64", layer(64, 160000, 64, [seg(160000, 64, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B64 M160000 N64 K448 J7 s1", DIRECT),
    ("dac16 B64", layer(64, 160000, 64, [seg(160000, 64)], alpha=1, res=1, res_rs=64, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B64 M160000 N64 K64 J1 s1", DIRECT),
    ("dac16 B64", layer(64, 160000, 64, [seg(160000, 64, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B64 M160000 N64 K448 J7 s1 d3", DIRECT),
    ("dac16 B64", layer(64, 160000, 64, [seg(160000, 64, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B64 M160000 N64 K448 J7 s1 d9", DIRECT),
    ("dac16 B64", layer(64, 80000, 128, [seg(160000, 64, J=2, pad=1, s=2)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M80000 N128 K256 J2 s2", 0),
    ("dac16 B64", layer(64, 80000, 128, [seg(80000, 128, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M80000 N128 K896 J7 s1", 0),
    ("dac16 B64", layer(64, 80000, 128, [seg(80000, 128)], alpha=1, res=1, res_rs=128, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M80000 N128 K128 J1 s1", 0),
    ("dac16 B64", layer(64, 80000, 128, [seg(80000, 128, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M80000 N128 K896 J7 s1 d3", 0),
    ("dac16 B64", layer(64, 80000, 128, [seg(80000, 128, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M80000 N128 K896 J7 s1 d9", 0),
    ("dac16 B64", layer(64, 20000, 256, [seg(80000, 128, J=2, pad=2, s=4)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M20000 N256 K1024 J2 s4", 0),
    ("dac16 B64", layer(64, 20000, 256, [seg(20000, 256, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M20000 N256 K1792 J7 s1", 0),
    ("dac16 B64", layer(64, 20000, 256, [seg(20000, 256)], alpha=1, res=1, res_rs=256, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M20000 N256 K256 J1 s1", 0),
    ("dac16 B64", layer(64, 20000, 256, [seg(20000, 256, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B64 M20000 N256 K1792 J7 s1 d3", 0),
    ("dac16 B64", layer(64, 20000, 256, [seg(20000, 256, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B64 M20000 N256 K1792 J7 s1 d9", 0),
    ("dac16 B64", layer(64, 4000, 512, [seg(20000, 256, J=2, pad=3, s=5)], alpha=1, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M4000 N512 K2560 J2 s5", 0),
    ("dac16 B64", layer(64, 4000, 512, [seg(4000, 512, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M4000 N512 K3584 J7 s1", 0),
    ("dac16 B64", layer(64, 4000, 512, [seg(4000, 512)], alpha=1, res=1, res_rs=512, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M4000 N512 K512 J1 s1", 0),
    ("dac16 B64", layer(64, 4000, 512, [seg(4000, 512, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B64 M4000 N512 K3584 J7 s1 d3", 0),
    ("dac16 B64", layer(64, 4000, 512, [seg(4000, 512, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B64 M4000 N512 K3584 J7 s1 d9", 0),
    ("dac16 B64", layer(64, 500, 1024, [seg(4000, 512, J=2, pad=4, s=8)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M500 N1024 K8192 J2 s8", 0),
    ("dac16 B64", layer(64, 500, 1024, [seg(500, 1024, J=3, pad=1)]), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M500 N1024 K3072 J3 s1", DIRECT),
    ("dac16 B64", layer(64, 500, 1536, [seg(500, 1024, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M500 N1536 K7168 J7 s1", 0),
    ("dac16 B64", layer(64, 501, 6144, [seg(500, 1536, J=2)], alpha=1, y_bs=3072000, y_elu=1, y_len=3072000, y_off=-3072), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M501 N6144 K3072 J2 s1", 0),
    ("dac16 B64", layer(64, 4000, 768, [seg(4000, 768, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M4000 N768 K5376 J7 s1", 0),
    ("dac16 B64", layer(64, 4000, 768, [seg(4000, 768)], alpha=1, res=1, res_rs=768, y_elu=1), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M4000 N768 K768 J1 s1", 0),
    ("dac16 B64", layer(64, 4000, 768, [seg(4000, 768, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B64 M4000 N768 K5376 J7 s1 d3", 0),
    ("dac16 B64", layer(64, 4000, 768, [seg(4000, 768, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B64 M4000 N768 K5376 J7 s1 d9", 0),
    ("dac16 B64", layer(64, 4001, 1920, [seg(4000, 768, J=2)], alpha=1, y_bs=7679616, y_elu=1, y_len=7679616, y_off=-1152), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M4001 N1920 K1536 J2 s1", 0),
    ("dac16 B64", layer(64, 19999, 384, [seg(19999, 384, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M19999 N384 K2688 J7 s1", 0),
    ("dac16 B64", layer(64, 19999, 384, [seg(19999, 384)], alpha=1, res=1, res_rs=384, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M19999 N384 K384 J1 s1", 0),
    ("dac16 B64", layer(64, 19999, 384, [seg(19999, 384, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B64 M19999 N384 K2688 J7 s1 d3", 0),
    ("dac16 B64", layer(64, 19999, 384, [seg(19999, 384, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B64 M19999 N384 K2688 J7 s1 d9", 0),
    ("dac16 B64", layer(64, 20000, 768, [seg(19999, 384, J=2)], alpha=1, y_bs=15359232, y_elu=1, y_len=15359232, y_off=-384), "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M20000 N768 K768 J2 s1", 0),
    ("dac16 B64", layer(64, 79996, 192, [seg(79996, 192, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B64 M79996 N192 K1344 J7 s1", 0),
    ("dac16 B64", layer(64, 79996, 192, [seg(79996, 192)], alpha=1, res=1, res_rs=192, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B64 M79996 N192 K192 J1 s1", 0),
    ("dac16 B64", layer(64, 79996, 192, [seg(79996, 192, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B64 M79996 N192 K1344 J7 s1 d3", 0),
    ("dac16 B64", layer(64, 79996, 192, [seg(79996, 192, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B64 M79996 N192 K1344 J7 s1 d9", 0),
    ("dac16 B64", layer(64, 79997, 192, [seg(79996, 192, J=2)], alpha=1, y_bs=15359232, y_elu=1, y_len=15359232, y_off=-96), "tap_gemm6_kernel<2, 2, 2, 3, 2> B64 M79997 N192 K384 J2 s1", 0),
    # dac16 B1
    ("dac16 B1", layer(1, 160000, 64, [seg(160000, 64, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M160000 N64 K448 J7 s1", DIRECT),
    ("dac16 B1", layer(1, 160000, 64, [seg(160000, 64)], alpha=1, res=1, res_rs=64, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M160000 N64 K64 J1 s1", DIRECT),
    ("dac16 B1", layer(1, 160000, 64, [seg(160000, 64, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M160000 N64 K448 J7 s1 d3", DIRECT),
    ("dac16 B1", layer(1, 160000, 64, [seg(160000, 64, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M160000 N64 K448 J7 s1 d9", DIRECT),
    ("dac16 B1", layer(1, 80000, 128, [seg(160000, 64, J=2, pad=1, s=2)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M80000 N128 K256 J2 s2", 0),
    ("dac16 B1", layer(1, 80000, 128, [seg(80000, 128, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M80000 N128 K896 J7 s1", 0),
    ("dac16 B1", layer(1, 80000, 128, [seg(80000, 128)], alpha=1, res=1, res_rs=128, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M80000 N128 K128 J1 s1", 0),
    ("dac16 B1", layer(1, 80000, 128, [seg(80000, 128, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M80000 N128 K896 J7 s1 d3", 0),
    ("dac16 B1", layer(1, 80000, 128, [seg(80000, 128, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M80000 N128 K896 J7 s1 d9", 0),
    ("dac16 B1", layer(1, 20000, 256, [seg(80000, 128, J=2, pad=2, s=4)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M20000 N256 K1024 J2 s4", 0),
    ("dac16 B1", layer(1, 20000, 256, [seg(20000, 256, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M20000 N256 K1792 J7 s1", 0),
    ("dac16 B1", layer(1, 20000, 256, [seg(20000, 256)], alpha=1, res=1, res_rs=256, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M20000 N256 K256 J1 s1", 0),
    ("dac16 B1", layer(1, 20000, 256, [seg(20000, 256, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M20000 N256 K1792 J7 s1 d3", 0),
    ("dac16 B1", layer(1, 20000, 256, [seg(20000, 256, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M20000 N256 K1792 J7 s1 d9", 0),
    ("dac16 B1", layer(1, 4000, 512, [seg(20000, 256, J=2, pad=3, s=5)], alpha=1, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N512 K2560 J2 s5", 0),
    ("dac16 B1", layer(1, 4000, 512, [seg(4000, 512, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N512 K3584 J7 s1", 0),
    ("dac16 B1", layer(1, 4000, 512, [seg(4000, 512)], alpha=1, res=1, res_rs=512, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N512 K512 J1 s1", 0),
    ("dac16 B1", layer(1, 4000, 512, [seg(4000, 512, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N512 K3584 J7 s1 d3", 0),
    ("dac16 B1", layer(1, 4000, 512, [seg(4000, 512, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N512 K3584 J7 s1 d9", 0),
    ("dac16 B1", layer(1, 500, 1024, [seg(4000, 512, J=2, pad=4, s=8)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M500 N1024 K8192 J2 s8", SPREAD),
    ("dac16 B1", layer(1, 500, 1024, [seg(500, 1024, J=3, pad=1)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M500 N1024 K3072 J3 s1", DIRECT | SPREAD),
    ("dac16 B1", layer(1, 500, 1536, [seg(500, 1024, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M500 N1536 K7168 J7 s1", SPREAD),
    ("dac16 B1", layer(1, 501, 6144, [seg(500, 1536, J=2)], alpha=1, y_bs=3072000, y_elu=1, y_len=3072000, y_off=-3072), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M501 N6144 K3072 J2 s1", 0),
    ("dac16 B1", layer(1, 4000, 768, [seg(4000, 768, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N768 K5376 J7 s1", 0),
    ("dac16 B1", layer(1, 4000, 768, [seg(4000, 768)], alpha=1, res=1, res_rs=768, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N768 K768 J1 s1", 0),
    ("dac16 B1", layer(1, 4000, 768, [seg(4000, 768, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N768 K5376 J7 s1 d3", 0),
    ("dac16 B1", layer(1, 4000, 768, [seg(4000, 768, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M4000 N768 K5376 J7 s1 d9", 0),
    ("dac16 B1", layer(1, 4001, 1920, [seg(4000, 768, J=2)], alpha=1, y_bs=7679616, y_elu=1, y_len=7679616, y_off=-1152), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M4001 N1920 K1536 J2 s1", 0),
    ("dac16 B1", layer(1, 19999, 384, [seg(19999, 384, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M19999 N384 K2688 J7 s1", 0),
    ("dac16 B1", layer(1, 19999, 384, [seg(19999, 384)], alpha=1, res=1, res_rs=384, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M19999 N384 K384 J1 s1", 0),
    ("dac16 B1", layer(1, 19999, 384, [seg(19999, 384, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B1 M19999 N384 K2688 J7 s1 d3", 0),
    ("dac16 B1", layer(1, 19999, 384, [seg(19999, 384, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B1 M19999 N384 K2688 J7 s1 d9", 0),
    ("dac16 B1", layer(1, 20000, 768, [seg(19999, 384, J=2)], alpha=1, y_bs=15359232, y_elu=1, y_len=15359232, y_off=-384), "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M20000 N768 K768 J2 s1", 0),
    ("dac16 B1", layer(1, 79996, 192, [seg(79996, 192, J=7, pad=3)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M79996 N192 K1344 J7 s1", 0),
    ("dac16 B1", layer(1, 79996, 192, [seg(79996, 192)], alpha=1, res=1, res_rs=192, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M79996 N192 K192 J1 s1", 0),
    ("dac16 B1", layer(1, 79996, 192, [seg(79996, 192, J=7, dil=3, pad=9)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B1 M79996 N192 K1344 J7 s1 d3", 0),
    ("dac16 B1", layer(1, 79996, 192, [seg(79996, 192, J=7, dil=9, pad=27)], alpha=1, y=0, y_elu=1), "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B1 M79996 N192 K1344 J7 s1 d9", 0),
    ("dac16 B1", layer(1, 79997, 192, [seg(79996, 192, J=2)], alpha=1, y_bs=15359232, y_elu=1, y_len=15359232, y_off=-96), "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M79997 N192 K384 J2 s1", 0),
    # wavtokenizer B1
    ("wavtokenizer B1", layer(1, 60000, 64, [seg(240000, 32, J=2, lim=240002, pad=2, s=4)]), "tap_gemm6_kernel<2, 2, 2, 1, 2> B1 M60000 N64 K256 J2 s4", 0),
    ("wavtokenizer B1", layer(1, 12000, 128, [seg(60000, 64, J=2, lim=60002, pad=3, s=5)]), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M12000 N128 K640 J2 s5", DIRECT),
    ("wavtokenizer B1", layer(1, 2400, 256, [seg(12000, 128, J=2, lim=12002, pad=3, s=5)], y_elu=1), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2400 N256 K1280 J2 s5", DIRECT | SPREAD),
    ("wavtokenizer B1", layer(1, 2400, 128, [seg(2400, 256, J=3, lim=2401, pad=1)], y=0, y_elu=1), "tap_gemm8_kernel<4, 2, 2, 2, 2> B1 M2400 N128 K768 J3 s1", DIRECT),
    ("wavtokenizer B1", layer(1, 2400, 256, [seg(2400, 128), seg(2400, 256, kofs=128)], y=0, y_elu=1), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M2400 N256 K384 J1 s1", DIRECT),
    ("wavtokenizer B1", layer(1, 400, 512, [seg(2400, 256, J=2, lim=2403, pad=3, s=6)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N512 K3072 J2 s6", DIRECT | SPREAD),
    ("wavtokenizer B1", layer(1, 400, 512, [seg(400, 512, J=7, lim=403, pad=3)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N512 K3584 J7 s1", DIRECT | SPREAD),
    ("wavtokenizer B1", layer(1, 400, 768, [seg(400, 512, J=7, pad=3)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N768 K3584 J7 s1", DIRECT | SPREAD),
    ("wavtokenizer B1", layer(1, 400, 768, [seg(400, 768, J=3, pad=1)]), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N768 K2304 J3 s1", DIRECT | SPREAD),
    ("wavtokenizer B1", layer(1, 400, 768, [seg(400, 768, J=3, pad=1)], res=1, res_rs=768), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N768 K2304 J3 s1", SPREAD),
    ("wavtokenizer B1", layer(1, 400, 2304, [seg(400, 768, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M400 N2304 K768 J1 s1", ROWMODE),
    ("wavtokenizer B1", layer(1, 400, 768, [seg(400, 768, bs=0)], res=1, res_rs=768, want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N768 K768 J1 s1", ROWMODE | SPREAD),
    ("wavtokenizer B1", layer(1, 400, 768, [seg(400, 2304, bs=0)], res=1, res_rs=768, scale=1, want_rowmode=1, y_bs=0), "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M400 N768 K2304 J1 s1", ROWMODE | SPREAD),
    ("wavtokenizer B1", layer(1, 400, 2432, [seg(400, 768, bs=0)], want_rowmode=1, y_bs=0), "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M400 N2432 K768 J1 s1", ROWMODE),
    ("wavtokenizer B1", layer(1, 403, 640, [seg(400, 2432, J=4)], n_valid=600, y_bs=240000, y_len=240000, y_off=-900, y_rs=600), "tap_gemm8_kernel<4, 2, 2, 2, 2> B1 M403 N640 K9728 J4 s1", 0),
    # encodec B1 exact
    ("encodec B1 exact", layer(1, 120000, 64, [seg(240000, 32, J=2, s=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 2, 2> B1 M120000 N64 K128 J2 s2", 0),
    ("encodec B1 exact", layer(1, 30000, 128, [seg(120000, 64, J=2, s=4)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M30000 N128 K512 J2 s4", 0),
    ("encodec B1 exact", layer(1, 30000, 64, [seg(30000, 128, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M30000 N64 K384 J3 s1", 0),
    ("encodec B1 exact", layer(1, 30000, 128, [seg(30000, 64), seg(30000, 128, kofs=64)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M30000 N128 K192 J1 s1", 0),
    ("encodec B1 exact", layer(1, 6000, 256, [seg(30000, 128, J=2, s=5)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6000 N256 K1280 J2 s5", 0),
    ("encodec B1 exact", layer(1, 6000, 128, [seg(6000, 256, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6000 N128 K768 J3 s1", 0),
    ("encodec B1 exact", layer(1, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6000 N256 K384 J1 s1", 0),
    ("encodec B1 exact", layer(1, 750, 512, [seg(6000, 256, J=2, s=8)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M750 N512 K4096 J2 s8", 0),
    ("encodec B1 exact", layer(1, 750, 2048, [seg(750, 512)], gemm_fp32=1, has_w6=0, has_winv=0, y_bs=2048), "tap_gemm4_kernel<2, 2, 4, 4> B1 M750 N2048 K512 J1 s1", 0),
    ("encodec B1 exact", layer(1, 750, 128, [seg(750, 512, J=7)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M750 N128 K3584 J7 s1", 0),
    ("encodec B1 exact", layer(1, 750, 512, [seg(750, 128, J=7)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M750 N512 K896 J7 s1", 0),
    ("encodec B1 exact", layer(1, 750, 2048, [seg(750, 512, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M750 N2048 K1024 J2 s1", 0),
    ("encodec B1 exact", layer(1, 6000, 640, [seg(6000, 256, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6000 N640 K512 J2 s1", 0),
    ("encodec B1 exact", layer(1, 30000, 256, [seg(30000, 128, J=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M30000 N256 K256 J2 s1", 0),
    ("encodec B1 exact", layer(1, 120000, 64, [seg(120000, 64, J=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 2, 2> B1 M120000 N64 K128 J2 s1", 0),
    # mimi B1 exact
    ("mimi B1 exact", layer(1, 60000, 128, [seg(240000, 64, J=2, s=4)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M60000 N128 K512 J2 s4", 0),
    ("mimi B1 exact", layer(1, 60000, 64, [seg(60000, 128, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M60000 N64 K384 J3 s1", 0),
    ("mimi B1 exact", layer(1, 60000, 128, [seg(60000, 64)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=128, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M60000 N128 K64 J1 s1", 0),
    ("mimi B1 exact", layer(1, 12000, 256, [seg(60000, 128, J=2, s=5)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M12000 N256 K1280 J2 s5", 0),
    ("mimi B1 exact", layer(1, 12000, 128, [seg(12000, 256, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M12000 N128 K768 J3 s1", 0),
    ("mimi B1 exact", layer(1, 12000, 256, [seg(12000, 128)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=256, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M12000 N256 K128 J1 s1", 0),
    ("mimi B1 exact", layer(1, 2000, 512, [seg(12000, 256, J=2, s=6)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2000 N512 K3072 J2 s6", 0),
    ("mimi B1 exact", layer(1, 2000, 256, [seg(2000, 512, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2000 N256 K1536 J3 s1", 0),
    ("mimi B1 exact", layer(1, 2000, 512, [seg(2000, 256)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=512, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2000 N512 K256 J1 s1", 0),
    ("mimi B1 exact", layer(1, 250, 1024, [seg(2000, 512, J=2, s=8)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N1024 K8192 J2 s8", 0),
    ("mimi B1 exact", layer(1, 250, 512, [seg(250, 1024, J=3)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N512 K3072 J3 s1", 0),
    ("mimi B1 exact", layer(1, 250, 1536, [seg(250, 512, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N1536 K512 J1 s1", 0),
    ("mimi B1 exact", layer(1, 250, 512, [seg(250, 512, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=512, scale=1, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N512 K512 J1 s1", 0),
    ("mimi B1 exact", layer(1, 250, 2048, [seg(250, 512, bs=0)], gelu=1, gemm_fp32=1, has_w6=0, has_winv=0, want_rowmode=1, want_rows=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N2048 K512 J1 s1", 0),
    ("mimi B1 exact", layer(1, 250, 512, [seg(250, 2048, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=512, scale=1, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N512 K2048 J1 s1", 0),
    ("mimi B1 exact", layer(1, 125, 512, [seg(250, 512, J=2, s=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M125 N512 K2048 J2 s2", 0),
    ("mimi B1 exact", layer(1, 250, 1024, [seg(250, 512, J=7)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N1024 K3584 J7 s1", 0),
    ("mimi B1 exact", layer(1, 250, 4096, [seg(250, 1024, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M250 N4096 K2048 J2 s1", 0),
    ("mimi B1 exact", layer(1, 2000, 1536, [seg(2000, 512, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2000 N1536 K1024 J2 s1", 0),
    ("mimi B1 exact", layer(1, 12000, 640, [seg(12000, 256, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M12000 N640 K512 J2 s1", 0),
    ("mimi B1 exact", layer(1, 60000, 256, [seg(60000, 128, J=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M60000 N256 K256 J2 s1", 0),
    # dac B1 exact
    ("dac B1 exact", layer(1, 441000, 64, [seg(441000, 64, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M441000 N64 K448 J7 s1", 0),
    ("dac B1 exact", layer(1, 441000, 64, [seg(441000, 64)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=64, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M441000 N64 K64 J1 s1", 0),
    ("dac B1 exact", layer(1, 441000, 64, [seg(441000, 64, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M441000 N64 K448 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 441000, 64, [seg(441000, 64, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M441000 N64 K448 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 220500, 128, [seg(441000, 64, J=2, pad=1, s=2)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M220500 N128 K256 J2 s2", 0),
    ("dac B1 exact", layer(1, 220500, 128, [seg(220500, 128, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M220500 N128 K896 J7 s1", 0),
    ("dac B1 exact", layer(1, 220500, 128, [seg(220500, 128)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=128, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M220500 N128 K128 J1 s1", 0),
    ("dac B1 exact", layer(1, 220500, 128, [seg(220500, 128, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M220500 N128 K896 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 220500, 128, [seg(220500, 128, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M220500 N128 K896 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 55125, 256, [seg(220500, 128, J=2, pad=2, s=4)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55125 N256 K1024 J2 s4", 0),
    ("dac B1 exact", layer(1, 55125, 256, [seg(55125, 256, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55125 N256 K1792 J7 s1", 0),
    ("dac B1 exact", layer(1, 55125, 256, [seg(55125, 256)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=256, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55125 N256 K256 J1 s1", 0),
    ("dac B1 exact", layer(1, 55125, 256, [seg(55125, 256, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55125 N256 K1792 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 55125, 256, [seg(55125, 256, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55125 N256 K1792 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 6890, 512, [seg(55125, 256, J=2, pad=4, s=8)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6890 N512 K4096 J2 s8", 0),
    ("dac B1 exact", layer(1, 6890, 512, [seg(6890, 512, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6890 N512 K3584 J7 s1", 0),
    ("dac B1 exact", layer(1, 6890, 512, [seg(6890, 512)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=512, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6890 N512 K512 J1 s1", 0),
    ("dac B1 exact", layer(1, 6890, 512, [seg(6890, 512, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6890 N512 K3584 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 6890, 512, [seg(6890, 512, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6890 N512 K3584 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 861, 1024, [seg(6890, 512, J=2, pad=4, s=8)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M861 N1024 K8192 J2 s8", 0),
    ("dac B1 exact", layer(1, 861, 1024, [seg(861, 1024, J=3, pad=1)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M861 N1024 K3072 J3 s1", 0),
    ("dac B1 exact", layer(1, 861, 1536, [seg(861, 1024, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M861 N1536 K7168 J7 s1", 0),
    ("dac B1 exact", layer(1, 862, 6144, [seg(861, 1536, J=2)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_bs=5289984, y_elu=1, y_len=5289984, y_off=-3072), "tap_gemm4_kernel<2, 2, 4, 4> B1 M862 N6144 K3072 J2 s1", 0),
    ("dac B1 exact", layer(1, 6888, 768, [seg(6888, 768, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6888 N768 K5376 J7 s1", 0),
    ("dac B1 exact", layer(1, 6888, 768, [seg(6888, 768)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=768, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6888 N768 K768 J1 s1", 0),
    ("dac B1 exact", layer(1, 6888, 768, [seg(6888, 768, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6888 N768 K5376 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 6888, 768, [seg(6888, 768, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6888 N768 K5376 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 6889, 3072, [seg(6888, 768, J=2)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_bs=21159936, y_elu=1, y_len=21159936, y_off=-1536), "tap_gemm4_kernel<2, 2, 4, 4> B1 M6889 N3072 K1536 J2 s1", 0),
    ("dac B1 exact", layer(1, 55104, 384, [seg(55104, 384, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55104 N384 K2688 J7 s1", 0),
    ("dac B1 exact", layer(1, 55104, 384, [seg(55104, 384)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=384, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55104 N384 K384 J1 s1", 0),
    ("dac B1 exact", layer(1, 55104, 384, [seg(55104, 384, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55104 N384 K2688 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 55104, 384, [seg(55104, 384, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55104 N384 K2688 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 55105, 768, [seg(55104, 384, J=2)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-384), "tap_gemm4_kernel<2, 2, 4, 4> B1 M55105 N768 K768 J2 s1", 0),
    ("dac B1 exact", layer(1, 220416, 192, [seg(220416, 192, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M220416 N192 K1344 J7 s1", 0),
    ("dac B1 exact", layer(1, 220416, 192, [seg(220416, 192)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=192, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M220416 N192 K192 J1 s1", 0),
    ("dac B1 exact", layer(1, 220416, 192, [seg(220416, 192, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M220416 N192 K1344 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 220416, 192, [seg(220416, 192, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M220416 N192 K1344 J7 s1 d9", 0),
    ("dac B1 exact", layer(1, 220417, 192, [seg(220416, 192, J=2)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y_bs=42319872, y_elu=1, y_len=42319872, y_off=-96), "tap_gemm4_kernel<2, 2, 4, 3> B1 M220417 N192 K384 J2 s1", 0),
    ("dac B1 exact", layer(1, 440832, 96, [seg(440832, 96, J=7, pad=3)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M440832 N96 K672 J7 s1", 0),
    ("dac B1 exact", layer(1, 440832, 96, [seg(440832, 96)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=96, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M440832 N96 K96 J1 s1", 0),
    ("dac B1 exact", layer(1, 440832, 96, [seg(440832, 96, J=7, dil=3, pad=9)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M440832 N96 K672 J7 s1 d3", 0),
    ("dac B1 exact", layer(1, 440832, 96, [seg(440832, 96, J=7, dil=9, pad=27)], alpha=1, gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 3> B1 M440832 N96 K672 J7 s1 d9", 0),
    # wavtokenizer B1 exact
    ("wavtokenizer B1 exact", layer(1, 240000, 16, [seg(240000, 32, J=3, lim=240001, pad=1)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<4, 1, 2, 1> B1 M240000 N16 K96 J3 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 240000, 32, [seg(240000, 16), seg(240000, 32, kofs=16)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm_kernel<4, 1, 2, 2, true>", 0),
    ("wavtokenizer B1 exact", layer(1, 60000, 64, [seg(240000, 32, J=2, lim=240002, pad=2, s=4)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M60000 N64 K256 J2 s4", 0),
    ("wavtokenizer B1 exact", layer(1, 60000, 32, [seg(60000, 64, J=3, lim=60001, pad=1)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<4, 1, 2, 2> B1 M60000 N32 K192 J3 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 60000, 64, [seg(60000, 32), seg(60000, 64, kofs=32)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M60000 N64 K96 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 12000, 128, [seg(60000, 64, J=2, lim=60002, pad=3, s=5)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M12000 N128 K640 J2 s5", 0),
    ("wavtokenizer B1 exact", layer(1, 12000, 64, [seg(12000, 128, J=3, lim=12001, pad=1)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B1 M12000 N64 K384 J3 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 12000, 128, [seg(12000, 64), seg(12000, 128, kofs=64)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M12000 N128 K192 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 2400, 256, [seg(12000, 128, J=2, lim=12002, pad=3, s=5)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2400 N256 K1280 J2 s5", 0),
    ("wavtokenizer B1 exact", layer(1, 2400, 128, [seg(2400, 256, J=3, lim=2401, pad=1)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2400 N128 K768 J3 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 2400, 256, [seg(2400, 128), seg(2400, 256, kofs=128)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B1 M2400 N256 K384 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 512, [seg(2400, 256, J=2, lim=2403, pad=3, s=6)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N512 K3072 J2 s6", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 2048, [seg(400, 512)], gemm_fp32=1, has_w6=0, has_winv=0, y_bs=2048), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N2048 K512 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 512, [seg(400, 512, J=7, lim=403, pad=3)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N512 K3584 J7 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 768, [seg(400, 512, J=7, pad=3)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N768 K3584 J7 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 768, [seg(400, 768, J=3, pad=1)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N768 K2304 J3 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 2304, [seg(400, 768, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N2304 K768 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 768, [seg(400, 768, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=768, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N768 K768 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 768, [seg(400, 2304, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, res=1, res_rs=768, scale=1, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N768 K2304 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 400, 2432, [seg(400, 768, bs=0)], gemm_fp32=1, has_w6=0, has_winv=0, want_rowmode=1, y_bs=0), "tap_gemm4_kernel<2, 2, 4, 4> B1 M400 N2432 K768 J1 s1", 0),
    ("wavtokenizer B1 exact", layer(1, 403, 640, [seg(400, 2432, J=4)], gemm_fp32=1, has_w6=0, has_winv=0, n_valid=600, y_bs=240000, y_len=240000, y_off=-900, y_rs=600), "tap_gemm4_kernel<2, 2, 4, 4> B1 M403 N640 K9728 J4 s1", 0),
    # encodec B64 exact
    ("encodec B64 exact", layer(64, 120000, 64, [seg(240000, 32, J=2, s=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 2, 2> B64 M120000 N64 K128 J2 s2", 0),
    ("encodec B64 exact", layer(64, 30000, 128, [seg(120000, 64, J=2, s=4)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M30000 N128 K512 J2 s4", 0),
    ("encodec B64 exact", layer(64, 30000, 64, [seg(30000, 128, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 2, 2> B64 M30000 N64 K384 J3 s1", 0),
    ("encodec B64 exact", layer(64, 30000, 128, [seg(30000, 64), seg(30000, 128, kofs=64)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M30000 N128 K192 J1 s1", 0),
    ("encodec B64 exact", layer(64, 6000, 256, [seg(30000, 128, J=2, s=5)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M6000 N256 K1280 J2 s5", 0),
    ("encodec B64 exact", layer(64, 6000, 128, [seg(6000, 256, J=3)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M6000 N128 K768 J3 s1", 0),
    ("encodec B64 exact", layer(64, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], gemm_fp32=1, has_w6=0, has_winv=0, y=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M6000 N256 K384 J1 s1", 0),
    ("encodec B64 exact", layer(64, 750, 512, [seg(6000, 256, J=2, s=8)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B64 M750 N512 K4096 J2 s8", 0),
    ("encodec B64 exact", layer(64, 750, 2048, [seg(750, 512)], gemm_fp32=1, has_w6=0, has_winv=0, y_bs=2048, y_rs=131072), "tap_gemm4_kernel<2, 2, 4, 4> B64 M750 N2048 K512 J1 s1", 0),
    ("encodec B64 exact", layer(64, 750, 128, [seg(750, 512, J=7)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B64 M750 N128 K3584 J7 s1", 0),
    ("encodec B64 exact", layer(64, 750, 512, [seg(750, 128, J=7)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B64 M750 N512 K896 J7 s1", 0),
    ("encodec B64 exact", layer(64, 750, 2048, [seg(750, 512, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M750 N2048 K1024 J2 s1", 0),
    ("encodec B64 exact", layer(64, 6000, 640, [seg(6000, 256, J=2)], gemm_fp32=1, has_w6=0, has_winv=0, y_elu=1), "tap_gemm4_kernel<2, 2, 4, 4> B64 M6000 N640 K512 J2 s1", 0),
    ("encodec B64 exact", layer(64, 30000, 256, [seg(30000, 128, J=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4> B64 M30000 N256 K256 J2 s1", 0),
    ("encodec B64 exact", layer(64, 120000, 64, [seg(120000, 64, J=2)], gemm_fp32=1, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 2, 2> B64 M120000 N64 K128 J2 s1", 0),
]

@pytest.mark.parametrize("case", LAYERS, ids=[f"{c[0]}-{c[2]}" for c in LAYERS])
def test_codec_layers(case):
    _, q, want, flags = case
    assert record(q) == (want, flags)



# The developer switches (ac_debug_set keys; the GPU tests use them as reference paths): layers whose launch each one changes,
# from the same workloads run with the switch set -- (case, layer with the switch, record without it, flags, record with it, flags)
SWITCHES = [
    # tap8=0
    ("encodec B64 tap8=0", layer(64, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap8=0),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT),
    ("encodec B64 tap8=0", layer(64, 750, 512, [seg(6000, 256, s=8, J=2)], tap8=0),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT | SPREAD, "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M750 N512 K4096 J2 s8", DIRECT),
    ("encodec B64 tap8=0", layer(64, 750, 128, [seg(750, 512, J=7)], tap8=0),
     "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M750 N128 K3584 J7 s1", DIRECT, "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M750 N128 K3584 J7 s1", DIRECT),
    # tap8=1
    ("encodec B64 tap8=1", layer(64, 30000, 128, [seg(120000, 64, s=4, J=2)], tap8=1),
     "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M30000 N128 K512 J2 s4", DIRECT, "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M30000 N128 K512 J2 s4", DIRECT),
    ("encodec B1 tap8=1", layer(1, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap8=1),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M6000 N256 K1280 J2 s5", DIRECT | SPREAD),
    ("mimi B1 tap8=1", layer(1, 12000, 256, [seg(12000, 128)], y=0, y_elu=1, res=1, res_rs=256, tap8=1),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M12000 N256 K128 J1 s1", 0, "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M12000 N256 K128 J1 s1", SPREAD),
    # tap8_form=1
    ("encodec B64 tap8_form=1", layer(64, 750, 512, [seg(6000, 256, s=8, J=2)], tap8_form=1),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT | SPREAD, "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT),
    ("mimi B1 tap8_form=1", layer(1, 2000, 512, [seg(2000, 256)], y=0, y_elu=1, res=1, res_rs=512, tap8_form=1),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N512 K256 J1 s1", SPREAD, "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M2000 N512 K256 J1 s1", 0),
    ("mimi B1 tap8_form=1", layer(1, 250, 1536, [seg(250, 512, bs=0)], y_bs=0, want_rowmode=1, tap8_form=1),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N1536 K512 J1 s1", ROWMODE | SPREAD, "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M250 N1536 K512 J1 s1", ROWMODE),
    # tap8_form=2
    ("encodec B64 tap8_form=2", layer(64, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap8_form=2),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT),
    ("encodec B64 tap8_form=2", layer(64, 750, 512, [seg(6000, 256, s=8, J=2)], tap8_form=2),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT | SPREAD, "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT),
    ("mimi B1 tap8_form=2", layer(1, 2000, 512, [seg(2000, 256)], y=0, y_elu=1, res=1, res_rs=512, tap8_form=2),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N512 K256 J1 s1", SPREAD, "tap_gemm8_kernel<4, 2, 2, 2, 2> B1 M2000 N512 K256 J1 s1", 0),
    # tap8_form=3
    ("encodec B64 tap8_form=3", layer(64, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap8_form=3),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT | SPREAD),
    ("dac B1 tap8_form=3", layer(1, 55125, 256, [seg(220500, 128, s=4, J=2, pad=2)], y_elu=1, alpha=1, tap8_form=3),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55125 N256 K1024 J2 s4", 0, "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M55125 N256 K1024 J2 s4", SPREAD),
    # tap8_spread=0
    ("encodec B64 tap8_spread=0", layer(64, 750, 512, [seg(6000, 256, s=8, J=2)], tap8_spread=0),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT | SPREAD, "tap_gemm8_kernel<2, 4, 2, 2, 2> B64 M750 N512 K4096 J2 s8", DIRECT),
    ("mimi B1 tap8_spread=0", layer(1, 2000, 512, [seg(2000, 256)], y=0, y_elu=1, res=1, res_rs=512, tap8_spread=0),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N512 K256 J1 s1", SPREAD, "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M2000 N512 K256 J1 s1", 0),
    ("mimi B1 tap8_spread=0", layer(1, 250, 1536, [seg(250, 512, bs=0)], y_bs=0, want_rowmode=1, tap8_spread=0),
     "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N1536 K512 J1 s1", ROWMODE | SPREAD, "tap_gemm8_kernel<2, 4, 2, 2, 2> B1 M250 N1536 K512 J1 s1", ROWMODE),
    # tap8_spread=2
    ("encodec B64 tap8_spread=2", layer(64, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap8_spread=2),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT | SPREAD),
    ("encodec B64 tap8_spread=2", layer(64, 750, 128, [seg(750, 512, J=7)], tap8_spread=2),
     "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M750 N128 K3584 J7 s1", DIRECT, "tap_gemm8_kernel<4, 2, 2, 2, 2> B64 M750 N128 K3584 J7 s1", DIRECT | SPREAD),
    ("dac B1 tap8_spread=2", layer(1, 55125, 256, [seg(220500, 128, s=4, J=2, pad=2)], y_elu=1, alpha=1, tap8_spread=2),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55125 N256 K1024 J2 s4", 0, "tap_gemm8_kernel<2, 4, 4, 2, 2> B1 M55125 N256 K1024 J2 s4", SPREAD),
    # tap_pick=0
    ("encodec B64 tap_pick=0", layer(64, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], y=0, y_elu=1, tap_pick=0),
     "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M6000 N256 K384 J1 s1", DIRECT, "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M6000 N256 K384 J1 s1", DIRECT),
    ("encodec B1 tap_pick=0", layer(1, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap_pick=0),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M6000 N256 K1280 J2 s5", DIRECT),
    ("mimi B1 tap_pick=0", layer(1, 12000, 256, [seg(12000, 128)], y=0, y_elu=1, res=1, res_rs=256, tap_pick=0),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M12000 N256 K128 J1 s1", 0, "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M12000 N256 K128 J1 s1", 0),
    # tap_pick=1
    ("encodec B1 tap_pick=1", layer(1, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap_pick=1),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm6_kernel<1, 4, 4, 2, 2> B1 M6000 N256 K1280 J2 s5", DIRECT),
    ("mimi B1 tap_pick=1", layer(1, 12000, 256, [seg(12000, 128)], y=0, y_elu=1, res=1, res_rs=256, tap_pick=1),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M12000 N256 K128 J1 s1", 0, "tap_gemm6_kernel<1, 4, 4, 2, 2> B1 M12000 N256 K128 J1 s1", 0),
    ("dac B1 tap_pick=1", layer(1, 6890, 512, [seg(6890, 512, J=7, dil=3, pad=9)], y=0, y_elu=1, alpha=1, tap_pick=1),
     "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6890 N512 K3584 J7 s1 d3", 0, "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B1 M6890 N512 K3584 J7 s1 d3", 0),
    # tap_pick=2
    ("encodec B64 tap_pick=2", layer(64, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], y=0, y_elu=1, tap_pick=2),
     "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M6000 N256 K384 J1 s1", DIRECT, "tap_gemm6_kernel<1, 8, 4, 1, 2> B64 M6000 N256 K384 J1 s1", DIRECT),
    ("dac B1 tap_pick=2", layer(1, 55125, 256, [seg(55125, 256, J=7, dil=3, pad=9)], y=0, y_elu=1, alpha=1, tap_pick=2),
     "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B1 M55125 N256 K1792 J7 s1 d3", 0, "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M55125 N256 K1792 J7 s1 d3", 0),
    ("dac B1 tap_pick=2", layer(1, 6889, 3072, [seg(6888, 768, J=2)], y_elu=1, alpha=1, y_bs=21159936, y_off=-1536, y_len=21159936, tap_pick=2),
     "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M6889 N3072 K1536 J2 s1", 0, "tap_gemm6_kernel<1, 8, 4, 1, 2> B1 M6889 N3072 K1536 J2 s1", 0),
    # tap_epi_staged=1
    ("encodec B64 tap_epi_staged=1", layer(64, 30000, 128, [seg(120000, 64, s=4, J=2)], tap_epi_staged=1),
     "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M30000 N128 K512 J2 s4", DIRECT, "tap_gemm6_kernel<1, 4, 4, 1, 2> B64 M30000 N128 K512 J2 s4", 0),
    ("encodec B64 tap_epi_staged=1", layer(64, 6000, 256, [seg(30000, 128, s=5, J=2)], y_elu=1, tap_epi_staged=1),
     "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", DIRECT, "tap_gemm8_kernel<2, 4, 4, 2, 2> B64 M6000 N256 K1280 J2 s5", 0),
    ("encodec B64 tap_epi_staged=1", layer(64, 6000, 256, [seg(6000, 128), seg(6000, 256, kofs=128)], y=0, y_elu=1, tap_epi_staged=1),
     "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M6000 N256 K384 J1 s1", DIRECT, "tap_gemm6_kernel<1, 4, 4, 2, 2> B64 M6000 N256 K384 J1 s1", 0),
    # tap_dil=0
    ("dac B1 tap_dil=0", layer(1, 55125, 256, [seg(55125, 256, J=7, dil=3, pad=9)], y=0, y_elu=1, alpha=1, tap_dil=0),
     "tap_gemm6_kernel<1, 4, 4, 2, 2, dil> B1 M55125 N256 K1792 J7 s1 d3", 0, "tap_gemm6_kernel<1, 4, 4, 2, 2> B1 M55125 N256 K1792 J7 s1 d3", 0),
    ("dac B1 tap_dil=0", layer(1, 55104, 384, [seg(55104, 384, J=7, dil=3, pad=9)], y=0, y_elu=1, alpha=1, tap_dil=0),
     "tap_gemm6_kernel<1, 4, 4, 1, 2, dil> B1 M55104 N384 K2688 J7 s1 d3", 0, "tap_gemm6_kernel<1, 4, 4, 1, 2> B1 M55104 N384 K2688 J7 s1 d3", 0),
    ("dac B1 tap_dil=0", layer(1, 220416, 192, [seg(220416, 192, J=7, dil=3, pad=9)], y=0, y_elu=1, alpha=1, tap_dil=0),
     "tap_gemm6_kernel<2, 2, 2, 3, 2, dil> B1 M220416 N192 K1344 J7 s1 d3", 0, "tap_gemm6_kernel<2, 2, 2, 3, 2> B1 M220416 N192 K1344 J7 s1 d3", 0),
]


@pytest.mark.parametrize("case", SWITCHES, ids=[c[0] for c in SWITCHES])
def test_switches(case):
    _, q, want0, flags0, want, flags = case
    assert record(dict(q, **SWITCH_DEFAULTS)) == (want0, flags0)
    assert record(q) == (want, flags)


# the exact-product kernels outside the split16 path: tap_gemm4 needs 16-byte aligned operands whose rows split into 32-float
# chunks; tap_gemm's vector form 16-byte aligned operands; anything else takes its scalar form
TAP8_LAYER = layer(64, 750, 512, [seg(750, 128, J=7)])             # EnCodec's decoder input conv: tap_gemm8 in the product path
EDGES = [
    ("exact products", dict(TAP8_LAYER, gemm_fp32=1), "tap_gemm4_kernel<2, 2, 4, 4>", 0),
    ("weights without split16 images", dict(TAP8_LAYER, has_w6=0, has_winv=0), "tap_gemm4_kernel<2, 2, 4, 4>", 0),
    ("split16 planes without scales", dict(TAP8_LAYER, has_winv=0), "tap_gemm6_kernel<1, 4, 4, 1, 2>", 0),
    ("per-clip lengths", layer(64, 750, 512, [seg(750, 128, J=7, rel_len=ALIGNED)]), "tap_gemm_kernel<2, 2, 4, 4, true>", 0),
    ("misaligned input", layer(64, 750, 512, [seg(750, 128, J=7, x=MISALIGNED)]), "tap_gemm_kernel<2, 2, 4, 4, false>", 0),
    ("misaligned weights", dict(TAP8_LAYER, w=MISALIGNED), "tap_gemm_kernel<2, 2, 4, 4, false>", 0),
    ("K % 4 != 0", layer(1, 400, 64, [seg(400, 1, J=7)]), "tap_gemm_kernel<2, 2, 2, 2, false>", 0),
    ("96 columns", layer(1, 400, 96, [seg(400, 3, J=7)]), "tap_gemm_kernel<2, 2, 4, 3, false>", 0),
    ("9 taps", layer(1, 400, 128, [seg(400, 128, J=9)]), "", REJECTED),
    ("9 taps, exact products", layer(1, 400, 128, [seg(400, 128, J=9)], gemm_fp32=1), "", REJECTED),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_edges(case):
    _, q, want, flags = case
    assert route(q) == (want, flags)


def test_rejects_bad_query():
    L = _built().lib()
    Q = Query()
    name = C.create_string_buffer(64)
    flags = C.c_int32()
    Q.nseg = 1
    assert L.ac_debug_tap_route(C.byref(Q), name, 64, C.byref(flags)) == -1          # struct_size unset
    Q.struct_size = C.sizeof(Query)
    Q.nseg = 3
    assert L.ac_debug_tap_route(C.byref(Q), name, 64, C.byref(flags)) == -1
    Q.nseg = 1
    assert L.ac_debug_tap_route(None, name, 64, C.byref(flags)) == -1
    assert L.ac_debug_tap_route(C.byref(Q), None, 64, C.byref(flags)) == -1
