"""The fp64 statement of STOI (audiocodecs_amd.stoi) in numpy, every step its own function, and the signals the
tests run on.  It restates pystoi's algorithm at its defaults (10 kHz, frames of 256 at hop 128, 512-point DFT, 15 third-octave bands
from 150 Hz, segments of 30 frames, -15 dB clipping, 40 dB silent-frame range) from its published description: pystoi is not on disk,
parity with it is unpinned.  The polyphase FIR is written out; tests/test_stoi_cpu.py pins it to scipy.signal.resample_poly.

x is the REFERENCE (clean) signal, y the hypothesis: x decides the silent frames, the clipping bound and the normalisation target.
Every function takes `dtype`: float64 is the statement, float32 the same steps in fp32 (what the kernel's tolerance is measured from)."""
import numpy as np

FS16, FS = 16000, 10000
UP, DOWN = 5, 8
HALF = 290                       # L: the FIR has 2 L + 1 = 581 taps
WIN, HOP, NFFT = 256, 128, 512
BANDS, SEG = 15, 30
DYN_RANGE = 40.0
EPS = 2.0 ** -52
CLIP = 1.0 + 10.0 ** (15.0 / 20.0)
EDGES = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138), (138, 174), (174, 219)]
KINDS = ("steady", "gaps", "late", "fade")
SNRS = (20.0, 10.0, 0.0)


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
def fir():
    """h[581] (fp64): pystoi's resample_oct(x, 10000, 16000) filter, normalised to sum 1 and multiplied by `up`."""
    fc = 1.0 / (2 * DOWN)
    df = fc / 10.0
    L = int(np.ceil((60.0 - 8.0) / (28.714 * df)))
    assert L == HALF
    beta = 0.1102 * (60.0 - 8.7)
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, beta) * (2 * UP * fc * np.sinc(2 * fc * t))
    return UP * h / h.sum()


def window():
    """hanning(258)[1:-1]: 256 samples, symmetric, no zero endpoints."""
    return np.hanning(WIN + 2)[1:-1]


def band_edges():
    """[(lo, hi)] * 15: the bins nearest 150 * 2^((2k -+ 1)/6) Hz on a grid of 10000 / 512 Hz."""
    f = np.linspace(0, FS, NFFT + 1)[: NFFT // 2 + 1]
    k = np.arange(BANDS)
    lo = 150.0 * 2.0 ** ((2 * k - 1) / 6.0)
    hi = 150.0 * 2.0 ** ((2 * k + 1) / 6.0)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo, hi)]


def dft_basis(dtype=np.float64):
    """[256, 2, 257]: w[n] cos / sin(2 pi k n / 512) -- the windowed 512-point DFT of a frame of 256 (the zero padding contributes nothing)."""
    n = np.arange(WIN)[:, None]
    k = np.arange(NFFT // 2 + 1)[None]
    a = 2.0 * np.pi * ((n * k) % NFFT) / NFFT
    w = window()[:, None]
    return np.stack([w * np.cos(a), w * np.sin(a)], axis=1).astype(dtype)


# ---- the steps ---------------------------------------------------------------------------------------------------------------------------
def num_frames(L16):
    L10 = -(-UP * L16 // DOWN)
    return (L10 - WIN) // HOP + 1 if L10 >= WIN else 0


def resample10k(x, dtype=np.float64):
    """x [L16] -> [ceil(5 L16 / 8)]: y[m] = sum_k h[8 m - 5 k + 290] x[k], zeros outside the signal."""
    x = np.asarray(x, dtype=dtype)
    h = fir().astype(dtype)
    L16 = x.shape[0]
    L10 = -(-UP * L16 // DOWN)
    y = np.zeros(L10, dtype=dtype)
    for p in range(UP):                               # outputs m = 5 i + p read x[8 i + d], d = -58 .. 64, with h[290 + 8 p - 5 d]
        d = np.arange(-58, 65)
        t = HALF + DOWN * p - UP * d
        taps = np.where((t >= 0) & (t <= 2 * HALF), h[np.clip(t, 0, 2 * HALF)], 0).astype(dtype)
        n_i = len(range(p, L10, UP))
        xp = np.zeros(DOWN * n_i + 123 + 58, dtype=dtype)
        xp[58:58 + L16] = x
        rows = np.lib.stride_tricks.as_strided(xp, shape=(n_i, 123), strides=(DOWN * xp.strides[0], xp.strides[0]))
        y[p::UP] = rows @ taps
    return y


def frame_energies(x10, dtype=np.float64):
    """e_f = 20 log10(||w x_f|| + EPS) over the frames of 256 at hop 128 that start at 0, 128, ... <= L10 - 256."""
    w = window().astype(dtype)
    F0 = (x10.shape[0] - WIN) // HOP + 1
    idx = HOP * np.arange(F0)[:, None] + np.arange(WIN)[None]
    fr = x10[idx] * w
    return (20.0 * np.log10(np.sqrt((fr * fr).sum(axis=1, dtype=dtype)) + dtype(EPS))).astype(dtype)


def silent_mask(e):
    """(kept [F0] bool, margin dB): keep e_f > max e - 40; margin is how far the nearest frame lies from the rule."""
    thr = e.max() - DYN_RANGE
    return e > thr, float(np.min(np.abs(e.astype(np.float64) - np.float64(thr))))


def rebuild(s10, kept, dtype=np.float64):
    """Overlap-add the kept windowed frames at hop 128: length (K - 1) 128 + 256."""
    w = window().astype(dtype)
    src = np.flatnonzero(kept)
    K = len(src)
    out = np.zeros((K - 1) * HOP + WIN if K else 0, dtype=dtype)
    for j, f in enumerate(src):
        out[HOP * j:HOP * j + WIN] += w * s10[HOP * f:HOP * f + WIN]
    return out


def envelopes(sig, dtype=np.float64):
    """[15, K - 1]: third-octave band envelopes of the STFT frames that start at 0, 128, ... < len - 256 (the last possible frame is left out)."""
    n = max(len(range(0, sig.shape[0] - WIN, HOP)), 0) if sig.shape[0] > WIN else 0
    idx = HOP * np.arange(n)[:, None] + np.arange(WIN)[None]
    fr = sig[idx] if n else np.zeros((0, WIN), dtype=dtype)
    bs = dft_basis(dtype)
    re, im = fr @ bs[:, 0], fr @ bs[:, 1]
    pw = re * re + im * im                                                        # [n, 257]
    return np.stack([np.sqrt(pw[:, lo:hi].sum(axis=1, dtype=dtype)) for lo, hi in EDGES]).astype(dtype)


def segment_values(X, Y, dtype=np.float64):
    """X, Y [15, n] -> [n - 29] (n >= 30): per segment the sum of the 15 band correlations divided by 15."""
    eps, clip = dtype(EPS), dtype(CLIP)
    win = np.lib.stride_tricks.sliding_window_view
    x, y = win(X, SEG, axis=1), win(Y, SEG, axis=1)                               # [15, n - 29, 30]: segment i holds the frames i .. i + 29
    c = np.sqrt((x * x).sum(axis=2, keepdims=True)) / (np.sqrt((y * y).sum(axis=2, keepdims=True)) + eps)
    yp = np.minimum(c * y, x * clip)
    xc = x - x.mean(axis=2, keepdims=True)
    yc = yp - yp.mean(axis=2, keepdims=True)
    xc = xc / (np.sqrt((xc * xc).sum(axis=2, keepdims=True)) + eps)
    yc = yc / (np.sqrt((yc * yc).sum(axis=2, keepdims=True)) + eps)
    return ((xc * yc).sum(axis=(0, 2), dtype=dtype) / dtype(BANDS)).astype(dtype)


def details(hyp, ref, dtype=np.float64):
    """hyp, ref [L16] at 16 kHz -> dict(score, kept [F0], K, S, segments [S], margin).  K - 1 < 30 gives 1e-5 (pystoi's warning path)."""
    dtype = np.dtype(dtype).type
    x, y = resample10k(ref, dtype), resample10k(hyp, dtype)
    kept, margin = silent_mask(frame_energies(x, dtype))
    K = int(kept.sum())
    if K - 1 < SEG:
        return dict(score=1e-5, kept=kept, K=K, S=0, segments=np.zeros(0, dtype=dtype), margin=margin)
    seg = segment_values(envelopes(rebuild(x, kept, dtype), dtype), envelopes(rebuild(y, kept, dtype), dtype), dtype)
    return dict(score=float(seg.sum(dtype=dtype) / dtype(len(seg))), kept=kept, K=K, S=len(seg), segments=seg, margin=margin)


def scores(hyp, ref, dtype=np.float64):
    """hyp, ref [B, L16] -> [B] fp64."""
    return np.array([details(h, r, dtype)["score"] for h, r in zip(np.atleast_2d(hyp), np.atleast_2d(ref))])


# ---- signals -----------------------------------------------------------------------------------------------------------------------------
def seed_of(L, b):
    """Clip b (1-based) of length L: the seed of its reference."""
    return 17 * L + 5 * b


def make_clip(kind, seed, L):
    """fp32 [L] at 16 kHz: 0.1 sum_{k=1..24} sin(2 pi 140 k t + phi_k) / k + N(0, 0.01), times the envelope of `kind`."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / FS16
    x = np.zeros(L)
    for k in range(1, 25):
        x += (0.1 / k) * np.sin(2.0 * np.pi * 140.0 * k * t + rng.uniform(0, 2 * np.pi))
    x += 0.01 * rng.standard_normal(L)
    phi = rng.uniform(0, 2 * np.pi)
    steady = 1.0 + 0.5 * np.sin(2.0 * np.pi * 4.0 * t + phi)
    if kind == "steady":
        env = steady
    elif kind == "gaps":
        env = np.where(np.mod(t, 0.17) < 0.12, 1.0, 10.0 ** (-70.0 / 20.0)) * (1.0 + 0.5 * np.sin(2.0 * np.pi * 3.0 * t))
    elif kind == "late":
        env = np.where(t < 0.1, 10.0 ** (-70.0 / 20.0), steady)
    elif kind == "fade":
        env = 10.0 ** (-4.0 * t / t[-1])
    else:
        raise ValueError(kind)
    return (x * env).astype(np.float32)


def make_ref(kind, L, B, first=1):
    """fp32 [B, L]: clips first .. first + B - 1 (the seeds 17 L + 5 b)."""
    return np.stack([make_clip(kind, seed_of(L, b), L) for b in range(first, first + B)])


def make_hyp(ref, L, p, first=1):
    """Hypothesis p of the clips `ref` [B, L]: ref + Gaussian noise at 20, 10, 0 dB SNR (of the clip's mean power) for p = 0, 1, 2."""
    out = np.empty_like(ref)
    for i, r in enumerate(ref):
        rng = np.random.default_rng(seed_of(L, first + i) + 7919 * (p + 1))
        rms = np.sqrt((r.astype(np.float64) ** 2).mean())
        out[i] = (r + rms * 10.0 ** (-SNRS[p] / 20.0) * rng.standard_normal(L)).astype(np.float32)
    return out
