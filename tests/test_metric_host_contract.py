"""The sizes the handle-free metrics' host code states -- every ac_*_tables_bytes, ac_*_packed_bytes, ac_*_workspace_bytes,
ac_*_num_frames, ac_knn_num_splits, ac_tokstats_state_bytes and ac_tokstats_form over a grid that crosses every refusal, every tile edge
and the 2^24 limit -- pinned to tests/golden/metric_host_contract.json, which was recorded from the library before the five metric
translation units were given one host-side scaffold (csrc/metric_host.h).  Pure host arithmetic: no GPU.

    python tests/test_metric_host_contract.py LIBRARY [OUT.json]

prints (or writes) the same record for any build of the library, to compare two builds or to record a deliberate change.  The fp64
sources of the tables (ac_*_source) are not pinned here: they depend on the machine's libm."""
import ctypes as C
import itertools
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metric_host_contract.json")

P_B = ((0, 1, 4, 5), (1, 3, 64))
KNN_ROWS, KNN_H = (1, 17, 5000), (32, 96, 512)
SPLITS = (0, 1, 64, 65)
# tests/test_tokstats_cpu.py: the shapes of test_form_is_a_pure_function_of_the_shape and of test_state_bytes_refuses
TOKSTATS = ((8, 1024), (8, 2048), (1, 16384), (1, 65536), (9, 1024), (3, 1000), (1, 4096), (64, 2), (1, 16385), (64, 1 << 20),
            (0, 1024), (-1, 1024), (65, 1024), (8, 1), (8, 0), (8, -5), (8, (1 << 20) + 1))
# function -> the argument tuples it is asked with, in order
GRID = {
    "ac_specdist_source_count": ((),), "ac_specdist_tables_bytes": ((),),
    "ac_stoi_source_count": ((),), "ac_stoi_tables_bytes": ((),),
    "ac_dnsmos_source_count": ((),), "ac_dnsmos_tables_bytes": ((),), "ac_dnsmos_weights_count": ((),), "ac_dnsmos_packed_bytes": ((),),
    "ac_specdist_num_frames": tuple((L,) for L in (512, 513, 5121, 160000, 1 << 24, (1 << 24) + 1)),
    "ac_specdist_workspace_bytes": tuple(itertools.product(*P_B, (512, 513, 5121, 160000, 1 << 24, (1 << 24) + 1))),
    "ac_stoi_num_frames": tuple((L,) for L in (1, 409, 410, 3000, 160000, 1 << 24, (1 << 24) + 1)),
    "ac_stoi_workspace_bytes": tuple(itertools.product(*P_B, (1, 409, 410, 3000, 160000, 1 << 24, (1 << 24) + 1))),
    "ac_dnsmos_workspace_bytes": tuple((S, H, W) for S in (0, 1, 3, 1025) for H, W in ((8, 8), (7, 8), (9, 15), (900, 120), (4096, 4096))),
    "ac_knn_packed_bytes": tuple(itertools.product(KNN_ROWS, KNN_H)),
    "ac_knn_num_splits": tuple(itertools.product(KNN_ROWS, KNN_ROWS, KNN_H, SPLITS)),
    "ac_knn_workspace_bytes": tuple(itertools.product(KNN_ROWS, KNN_ROWS, KNN_H, (0, 4, 8, 9), SPLITS)),
    "ac_tokstats_state_bytes": TOKSTATS,
    "ac_tokstats_form": TOKSTATS,
}


def record(L):
    return {name: [int(getattr(L, name)(*args)) for args in grid] for name, grid in GRID.items()}


def test_sizes_are_those_recorded():
    from audiocodecs_amd import _native

    with open(GOLDEN) as f:
        want = json.load(f)
    got = record(_native.lib())
    assert sorted(got) == sorted(want)
    for name, grid in GRID.items():
        assert len(want[name]) == len(grid), name
        wrong = [(args, g, w) for args, g, w in zip(grid, got[name], want[name]) if g != w]
        assert not wrong, f"{name}: (arguments, returned, recorded) {wrong[:5]}"


if __name__ == "__main__":
    from audiocodecs_amd import _native

    L = C.CDLL(sys.argv[1])
    for name in GRID:
        getattr(L, name).restype, getattr(L, name).argtypes = _native.EXPORTS[name]
    text = json.dumps(record(L), separators=(",", ":")).replace('],"', '],\n"') + "\n"
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
