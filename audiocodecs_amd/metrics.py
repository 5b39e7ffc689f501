"""STFT and mel spectral distances: the two resynthesis metrics every evaluation recipe of the reference appends
(the reference's downstream/metrics/stft_distance.py, mel_distance.py; downstream/test_sr.py:102-142) as one call.

``spectral_distances(hyp_sig, ref_sig, sample_rate)`` resamples both signals to 16 kHz (``audiocodecs_amd.resample``) and returns, per
clip, the mean over frames of the L2 norm of the dB difference of the two magnitude spectrograms (513 bins) and of the two mel
spectrograms (80 mels).  It runs in the HIP library (``ac_specdist``): one split16 MFMA GEMM per tile of 16 frames
with the dB, mel and norm steps in registers -- no spectrogram reaches memory; there is no CPU fallback.  Only the reference's
defaults are compiled: n_fft = win_length = 1024, hop 320, periodic Hann window, center = True with reflect padding, 80 HTK mel
filters over 0 .. 8000 Hz without norm, dB = 10 log10(max(x, 1e-10)) without top_db.

``STFTDistance`` and ``MelDistance`` have the reference classes' constructor and ``append``; of speechbrain's ``MetricStats`` only the
subset below exists (``ids``, ``scores``, ``clear``, ``summarize``).

**Parity with torchaudio's MelSpectrogram / AmplitudeToDB is unpinned**: torchaudio is not on disk, the filterbank and the dB rule are
restated from its published algorithm.  The STFT part is pinned to ``torch.stft``, which is what the reference calls.

``stoi(hyp_sig, ref_sig, sample_rate)`` is the third signal-processing metric of those recipes (downstream/metrics/stoi.py: torchmetrics
calling pystoi clip by clip on the host) as one call on the device (``ac_stoi``): both signals to 16 kHz, pystoi's
second resampling to 10 kHz, the removal of the frames more than 40 dB below the reference's loudest, overlap-add, a 512-point STFT as a
split16 MFMA GEMM, 15 third-octave band envelopes and the clipped, normalised correlation over segments of 30 frames.  The number of kept
frames is never read back by the host.  ``ref_sig`` is pystoi's clean signal x: the score is not symmetric.  Only ``extended=False`` is
compiled.  ``STOI`` has the reference class's constructor and ``append``.

**Parity with pystoi is unpinned**: neither pystoi nor torchmetrics is on disk; the FIR, the window, the band edges and every step are
restated from pystoi's published algorithm (tests/stoi_ref.py is that statement in fp64; the FIR is pinned to scipy.signal.resample_poly).
"""

from __future__ import annotations

import torch

from . import _metric_host as _host
from . import _native
from ._metric_host import MAX_HYPS, SAMPLE_RATE

__all__ = ["spectral_distances", "STFTDistance", "MelDistance", "stoi", "STOI", "num_frames", "stoi_num_frames", "SAMPLE_RATE", "N_FFT", "HOP_LENGTH", "N_MELS", "MAX_HYPS"]

N_FFT = 1024
HOP_LENGTH = 320
N_MELS = 80


def _check_defaults(n_fft=N_FFT, hop_length=HOP_LENGTH, n_mels=N_MELS) -> None:
    if (n_fft, hop_length, n_mels) != (N_FFT, HOP_LENGTH, N_MELS):
        raise ValueError(f"only the reference's defaults are compiled: n_fft={N_FFT}, hop_length={HOP_LENGTH}, n_mels={N_MELS} "
                         f"(got n_fft={n_fft}, hop_length={hop_length}, n_mels={n_mels})")


def num_frames(length_16k: int) -> int:
    """Frames of a signal of `length_16k` samples at 16 kHz: 1 + L // 320 (center = True)."""
    if length_16k <= N_FFT // 2:
        raise ValueError(f"a signal of {length_16k} samples at {SAMPLE_RATE} Hz cannot be reflect-padded by {N_FFT // 2}: it must be longer than that")
    return 1 + int(length_16k) // HOP_LENGTH


def _pair_at_16k(hyp_sig, ref_sig, sample_rate, n):
    """The refusals that look at the devices, then both signals at 16 kHz, fp32 and contiguous: (hyp [n * B, L16], ref [B, L16])."""
    from .resample import resample

    _host.need_cuda(hyp_sig.is_cuda and ref_sig.is_cuda, "metrics", "signals")
    if hyp_sig.device != ref_sig.device:
        raise ValueError(f"`hyp_sig` is on {hyp_sig.device}, `ref_sig` on {ref_sig.device}")
    ref = resample(ref_sig.detach().to(torch.float32), sample_rate, SAMPLE_RATE).contiguous()
    hyp = resample(hyp_sig.detach().to(torch.float32).reshape(n * ref_sig.shape[0], ref_sig.shape[1]), sample_rate, SAMPLE_RATE).contiguous()
    return hyp, ref


@torch.no_grad()
def spectral_distances(hyp_sig: torch.Tensor, ref_sig: torch.Tensor, sample_rate: int, return_frames: bool = False):
    """hyp_sig [B, T] (or [P, B, T]: P hypotheses of the same clips), ref_sig [B, T], both at `sample_rate` -> (stft, mel), each [B]
    (or [P, B]) fp32 on the signals' device.  With `return_frames` also the per-frame distances the scores are the means of:
    (stft, mel, stft_frames, mel_frames), the last two [B, F] (or [P, B, F]).  The rows of a [P, B, T] call are bit for bit those of P
    separate calls; a clip that holds an inf or a NaN gets NaN scores and disturbs no other clip."""
    P, B, _, L16 = _host.check_pair(hyp_sig, ref_sig, sample_rate)
    dev = ref_sig.device
    lead = () if P is None else (P,)
    F = num_frames(L16)
    if B == 0:            # an empty shard: the empty result (the library is not called)
        out = tuple(torch.empty(lead + (0,), dtype=torch.float32, device=dev) for _ in range(2))
        return out + tuple(torch.empty(lead + (0, F), dtype=torch.float32, device=dev) for _ in range(2)) if return_frames else out
    n = 1 if P is None else P
    hyp, ref = _pair_at_16k(hyp_sig, ref_sig, sample_rate, n)
    tables = _host.tables("specdist", dev)
    stft = torch.empty(n, B, dtype=torch.float32, device=dev)
    mel = torch.empty(n, B, dtype=torch.float32, device=dev)
    sfr = torch.empty(n, B, F, dtype=torch.float32, device=dev) if return_frames else None
    mfr = torch.empty(n, B, F, dtype=torch.float32, device=dev) if return_frames else None
    ws = _host.sized_buffer("ac_specdist_workspace_bytes", dev, P=n, B=B, L=L16)
    ptr = _native._ptr
    with torch.cuda.device(dev):
        rc = _native.lib().ac_specdist(ptr(hyp), ptr(ref), n, B, L16, ptr(tables), ptr(stft), ptr(mel), ptr(sfr), ptr(mfr), ptr(ws), ws.numel(), _native._stream())
    _native.check(rc, None, "ac_specdist")
    shape = lead + (B,)
    if return_frames:
        return stft.reshape(shape), mel.reshape(shape), sfr.reshape(shape + (F,)), mfr.reshape(shape + (F,))
    return stft.reshape(shape), mel.reshape(shape)


class _DistanceStats:
    """The bookkeeping of speechbrain's ``MetricStats`` that the reference's recipes use, and nothing else: ``ids`` and ``scores``
    (lists, one entry per appended clip), ``clear()`` and ``summarize(field=None)`` with the fields ``average``, ``min_score``,
    ``min_id``, ``max_score``, ``max_id``.  There is no ``write_stats``, no batch evaluation, no ``n_jobs``."""

    _which = 0           # index into spectral_distances' result

    def clear(self) -> None:
        self.ids = []
        self.scores = []
        self.summary = {}

    @torch.no_grad()
    def append(self, ids, hyp_sig, ref_sig, lens=None):
        """`lens` is accepted and ignored, as the reference ignores it."""
        if not torch.is_tensor(hyp_sig) or not torch.is_tensor(ref_sig) or hyp_sig.shape != ref_sig.shape or hyp_sig.dim() != 2:
            raise ValueError("`hyp_sig` and `ref_sig` must be [B, T] tensors of the same shape")
        self._record(ids, hyp_sig.shape[0], lambda: self._scores(hyp_sig, ref_sig))

    def _record(self, ids, B, scores) -> None:
        """One id per clip, then `scores()` [B] behind them."""
        ids = list(ids)
        if len(ids) != B:
            raise ValueError(f"{len(ids)} ids for {B} clips")
        scores = scores()
        self.ids += ids
        self.scores += scores.cpu().tolist()

    def _scores(self, hyp_sig, ref_sig):
        return spectral_distances(hyp_sig, ref_sig, self.sample_rate)[self._which]

    def summarize(self, field=None):
        if not self.scores:
            raise ValueError("summarize: nothing was appended")
        lo = min(range(len(self.scores)), key=self.scores.__getitem__)
        hi = max(range(len(self.scores)), key=self.scores.__getitem__)
        self.summary = {
            "average": float(sum(self.scores) / len(self.scores)),
            "min_score": float(self.scores[lo]),
            "min_id": self.ids[lo],
            "max_score": float(self.scores[hi]),
            "max_id": self.ids[hi],
        }
        return self.summary if field is None else self.summary[field]


class STFTDistance(_DistanceStats):
    """downstream/metrics/stft_distance.py: per clip the mean over frames of the L2 norm over the 513 bins of the dB difference of the
    two magnitude spectrograms.  Only the subset of ``MetricStats`` that `_DistanceStats` states exists."""

    __doc__ += _DistanceStats.__doc__
    _which = 0

    def __init__(self, sample_rate, n_fft=N_FFT, hop_length=HOP_LENGTH):
        _check_defaults(n_fft=n_fft, hop_length=hop_length)
        self.sample_rate, self.n_fft, self.hop_length = sample_rate, n_fft, hop_length
        self.clear()


class MelDistance(_DistanceStats):
    """downstream/metrics/mel_distance.py: per clip the mean over frames of the L2 norm over the 80 mels of the dB difference of the
    two mel spectrograms (power 1).  Only the subset of ``MetricStats`` that `_DistanceStats` states exists."""

    __doc__ += _DistanceStats.__doc__
    _which = 1

    def __init__(self, sample_rate, n_mels=N_MELS, n_fft=N_FFT, hop_length=HOP_LENGTH):
        _check_defaults(n_fft=n_fft, hop_length=hop_length, n_mels=n_mels)
        self.sample_rate, self.n_mels, self.n_fft, self.hop_length = sample_rate, n_mels, n_fft, hop_length
        self.clear()


# ---- STOI ------------------------------------------------------------------------------------------------------------------------------
STOI_MIN_LEN_10K = 256          # one frame at 10 kHz
STOI_SEGMENT = 30               # frames per segment


def stoi_num_frames(length_16k: int) -> int:
    """Frames of 256 at hop 128 of a signal of `length_16k` samples at 16 kHz once it stands at 10 kHz (before the silent ones go):
    (ceil(5 L / 8) - 256) // 128 + 1."""
    L10 = -(-5 * int(length_16k) // 8)
    if L10 < STOI_MIN_LEN_10K:
        raise ValueError(f"a signal of {length_16k} samples at {SAMPLE_RATE} Hz is {L10} samples at 10 kHz: STOI needs one frame of {STOI_MIN_LEN_10K}")
    return (L10 - STOI_MIN_LEN_10K) // 128 + 1


@torch.no_grad()
def stoi(hyp_sig: torch.Tensor, ref_sig: torch.Tensor, sample_rate: int, extended: bool = False, return_details: bool = False):
    """hyp_sig [B, T] (or [P, B, T]: P hypotheses of the same clips), ref_sig [B, T] (the clean signal), both at `sample_rate` -> the STOI
    score [B] (or [P, B]) fp32 on the signals' device.  With `return_details` (score, kept, num_segments, segments): kept [B, F0] bool,
    the frames the silent-frame rule keeps; num_segments [B] int32; segments [B, max(F0 - 30, 0)] (or [P, B, ...]) fp32, per segment the
    sum of the 15 band correlations / 15, NaN past num_segments.  Fewer than 30 frames left give 1e-5, as pystoi does.  The rows of a
    [P, B, T] call are bit for bit those of P separate calls; a clip that holds an inf or a NaN gets a NaN score and disturbs no other."""
    if extended is not False:
        raise ValueError(f"only the reference's default is compiled: extended=False (got extended={extended!r})")
    P, B, _, L16 = _host.check_pair(hyp_sig, ref_sig, sample_rate)
    F0 = stoi_num_frames(L16)
    dev = ref_sig.device
    lead = () if P is None else (P,)
    NS0 = max(F0 - STOI_SEGMENT, 0)
    if B == 0:            # an empty shard: the empty result (the library is not called)
        score = torch.empty(lead + (0,), dtype=torch.float32, device=dev)
        if not return_details:
            return score
        return (score, torch.empty(0, F0, dtype=torch.bool, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(lead + (0, NS0), dtype=torch.float32, device=dev))
    n = 1 if P is None else P
    hyp, ref = _pair_at_16k(hyp_sig, ref_sig, sample_rate, n)
    tables = _host.tables("stoi", dev)
    score = torch.empty(n, B, dtype=torch.float32, device=dev)
    kept = torch.empty(B, F0, dtype=torch.bool, device=dev) if return_details else None
    nseg = torch.empty(B, dtype=torch.int32, device=dev) if return_details else None
    segs = torch.empty(n, B, NS0, dtype=torch.float32, device=dev) if return_details else None
    ws = _host.sized_buffer("ac_stoi_workspace_bytes", dev, P=n, B=B, L16=L16)
    ptr = _native._ptr
    with torch.cuda.device(dev):
        rc = _native.lib().ac_stoi(ptr(hyp), ptr(ref), n, B, L16, ptr(tables), ptr(score), ptr(kept), ptr(nseg), ptr(segs), ptr(ws), ws.numel(), _native._stream())
    _native.check(rc, None, "ac_stoi")
    shape = lead + (B,)
    if return_details:
        return score.reshape(shape), kept, nseg, segs.reshape(shape + (NS0,))
    return score.reshape(shape)


class STOI(_DistanceStats):
    """downstream/metrics/stoi.py: per clip the short-time objective intelligibility of `hyp_sig` against the clean `ref_sig` (pystoi's
    defaults, extended = False).  Only the subset of ``MetricStats`` that `_DistanceStats` states exists."""

    __doc__ += _DistanceStats.__doc__

    def __init__(self, sample_rate):
        self.sample_rate = sample_rate
        self.clear()

    def _scores(self, hyp_sig, ref_sig):
        return stoi(hyp_sig, ref_sig, self.sample_rate)
