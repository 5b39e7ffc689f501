// metric_host.h: the host side that the five handle-free metric translation units share (knn.hip, specdist.hip, stoi.hip, dnsmos.hip,
// tokstats.hip).  Host code only: no kernel and nothing a kernel calls.  A metric keeps what is its own -- its shape
// rule, its frequency points, its launches -- and takes from here the pointer alignment rule, the status an entry point returns behind
// its launches, the fp64 cosine of its DFT table, the triangular filters of its mel table and the cursor that lays out its workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "audiocodecs_amd.h"

namespace ac {

// a null pointer is aligned: an optional argument is checked like a given one
template <int BYTES>
static bool aligned(const void* p) {
    static_assert(BYTES == 4 || BYTES == 8 || BYTES == 16, "the alignments the entry points promise");
    return (reinterpret_cast<uintptr_t>(p) & (BYTES - 1)) == 0;
}

// what an entry point returns behind its launches
static int launch_status() { return hipGetLastError() == hipSuccess ? AC_OK : AC_EHIP; }

// cos(2 pi j / n), n a multiple of 8, 0 <= j < n, with the argument reduced to the first octant as an integer: exact at the multiples of
// a quarter turn
static double cos_turn(int j, int n) {
    const int quarter = n / 4, q = j / quarter, r = j % quarter;
    const double u = M_PI / (n / 2);
    const double cs = r <= quarter / 2 ? cos(r * u) : sin((quarter - r) * u), sn = r <= quarter / 2 ? sin(r * u) : cos((quarter - r) * u);
    return q == 0 ? cs : q == 1 ? -sn : q == 2 ? -cs : sn;
}

// fb[bins][mels]: filter m is the triangle over f_pts[m] .. f_pts[m + 2] with its peak at f_pts[m + 1], read at the bins' frequencies
// f_bin[bins]; with `slaney_norm` every filter is scaled to the area 2 / (f_pts[m + 2] - f_pts[m]) (librosa's norm = "slaney")
static void triangle_filterbank(double* fb, const double* f_pts, int mels, const double* f_bin, int bins, bool slaney_norm) {
    for (int k = 0; k < bins; ++k) {
        const double f = f_bin[k];
        for (int m = 0; m < mels; ++m) {
            const double down = (f - f_pts[m]) / (f_pts[m + 1] - f_pts[m]), up = (f_pts[m + 2] - f) / (f_pts[m + 2] - f_pts[m + 1]);
            const double v = down < up ? down : up;
            fb[k * mels + m] = v > 0.0 ? (slaney_norm ? v * 2.0 / (f_pts[m + 2] - f_pts[m]) : v) : 0.0;
        }
    }
}

// Lays the pieces of a workspace out one behind the other, every piece at a multiple of ALIGN: take() returns the piece's offset, `at`
// is the size so far.
template <size_t ALIGN>
struct WorkspaceCursor {
    size_t at = 0;
    size_t take(size_t bytes) {
        const size_t o = at;
        at += (bytes + ALIGN - 1) / ALIGN * ALIGN;
        return o;
    }
};

}  // namespace ac
