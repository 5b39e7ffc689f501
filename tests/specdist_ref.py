"""The fp64 statement of the STFT and mel spectral distances (audiocodecs_amd.metrics) and the signals the tests
run on.  Explicit reflect padding and framing, numpy.fft.rfft, torchaudio's HTK filterbank restated from its formula; nothing here
calls torch.stft (tests/test_specdist_cpu.py pins this file to it, and to the fixture tools/make_specdist_golden.py wrote)."""
import numpy as np

N_FFT, HOP, N_MELS, SR = 1024, 320, 80, 16000
BINS = N_FFT // 2 + 1
KINDS = ("floor", "noise", "dynamic")


def window():
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT))      # periodic Hann (torch.hann_window's default)


def filterbank():
    """[513, 80]: triangular filters on the HTK mel scale over 0 .. 8000 Hz, norm=None."""
    all_freqs = np.linspace(0.0, SR // 2, BINS)
    m_pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + (SR // 2) / 700.0), N_MELS + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_pts[-1] = SR // 2          # the last point maps back to f_max by definition (the formula leaves 8000 + 5e-12, and 7e-15 in row 512)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up))


def frames(sig):
    """sig [B, L] -> [B, F, 1024]: frame f covers samples 320 f - 512 .. 320 f + 511 of the reflect-padded signal."""
    sig = np.asarray(sig, dtype=np.float64)
    L = sig.shape[-1]
    if L <= N_FFT // 2:
        raise ValueError(f"a signal of {L} samples cannot be reflect-padded by {N_FFT // 2}")
    padded = np.concatenate([sig[:, N_FFT // 2:0:-1], sig, sig[:, -2:-N_FFT // 2 - 2:-1]], axis=1)
    F = 1 + L // HOP
    idx = HOP * np.arange(F)[:, None] + np.arange(N_FFT)[None]
    return padded[:, idx]


def magnitudes(sig):
    """[B, L] -> |STFT| [B, F, 513] in fp64."""
    return np.abs(np.fft.rfft(frames(sig) * window(), axis=-1))


def db(x):
    return 10.0 * np.log10(np.maximum(x, 1e-10))      # AmplitudeToDB's defaults: multiplier 10 (even on magnitudes), amin 1e-10, no top_db


def distances(hyp, ref):
    """hyp, ref [B, L] at 16 kHz -> (stft [B], mel [B], stft_frames [B, F], mel_frames [B, F]) in fp64."""
    mh, mr = magnitudes(hyp), magnitudes(ref)
    fb = filterbank()
    sf = np.sqrt(((db(mh) - db(mr)) ** 2).sum(axis=-1))
    mf = np.sqrt(((db(mh @ fb) - db(mr @ fb)) ** 2).sum(axis=-1))
    return sf.mean(axis=-1), mf.mean(axis=-1), sf, mf


def torch_fp32(hyp, ref):
    """The reference's own arithmetic in fp32 on the CPU (torch.stft, fp32 matmul, log10): what the kernel's tolerance is measured from."""
    import torch

    fb = torch.from_numpy(filterbank()).float()
    win = torch.hann_window(N_FFT)

    def both(x):
        m = torch.stft(torch.from_numpy(np.asarray(x, dtype=np.float32)), n_fft=N_FFT, hop_length=HOP, window=win, return_complex=True).abs()    # [B, 513, F]
        a2db = lambda v: 10.0 * torch.log10(torch.clamp(v, min=1e-10))
        return a2db(m), a2db(torch.matmul(m.transpose(-1, -2), fb).transpose(-1, -2))

    (sh, mh), (sr, mr) = both(hyp), both(ref)
    sf, mf = (sh - sr).norm(dim=1), (mh - mr).norm(dim=1)
    return sf.mean(dim=1).numpy(), mf.mean(dim=1).numpy(), sf.numpy(), mf.numpy()


# ---- signals ---------------------------------------------------------------------------------------------------------------------------
def make_signal(kind, seed, B, L):
    """fp32 [B, L].  floor: 29 harmonics of 110 (b + 1) Hz at amplitude 0.1 / k plus Gaussian noise at 1e-3; noise: Gaussian at 0.1;
    dynamic: floor with its second half scaled by 2^-14.  Every bin of every frame stands well above the fp32 rounding floor."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (0.1 * rng.standard_normal((B, L))).astype(np.float32)
    t = np.arange(L) / SR
    x = np.zeros((B, L))
    for b in range(B):
        for k in range(1, 30):
            x[b] += (0.1 / k) * np.sin(2.0 * np.pi * 110.0 * (b + 1) * k * t + rng.uniform(0, 2 * np.pi))
    x += 1e-3 * rng.standard_normal((B, L))
    if kind == "dynamic":
        x[:, L // 2:] *= 2.0 ** -14
    elif kind != "floor":
        raise ValueError(kind)
    return x.astype(np.float32)


def make_pair(kind, seed, B, L, hyp=0):
    """(hyp, ref): hyp = ref + 1 % noise -- Gaussian at 1 % of the clip's rms, the same level over the whole clip (in the quiet half
    of `dynamic` the noise lies far above the signal: the distance there is large and rests on the dB of the quiet reference).
    `hyp` numbers the hypotheses of one reference: each has its own noise."""
    ref = make_signal(kind, seed, B, L)
    rng = np.random.default_rng(seed + 7919 * (hyp + 1))
    n = 0.01 * np.sqrt((ref.astype(np.float64) ** 2).mean(axis=1, keepdims=True)) * rng.standard_normal((B, L))
    return (ref + n).astype(np.float32), ref


def null_margin(sig):
    """The smallest magnitude of any (frame, bin) of sig [B, L] as a fraction of its frame's largest."""
    m = magnitudes(sig)
    return float((m.min(axis=-1) / m.max(axis=-1)).min())


def rel_err(got, want):
    """Largest |got - want| / |want| (distances between different signals are far from 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))
