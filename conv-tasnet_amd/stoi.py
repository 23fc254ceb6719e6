"""Short-time objective intelligibility: STOI and ESTOI without pystoi.

Speech-separation papers report STOI (C. Taal, R. Hendriks, R. Heusdens, J. Jensen, "An
algorithm for intelligibility prediction of time-frequency weighted noisy speech", IEEE
TASLP 19(7), 2011) and ESTOI (J. Jensen, C. Taal, "An algorithm for predicting the
intelligibility of speech masked by modulated noise maskers", IEEE TASLP 24(11), 2016) next
to SI-SNRi and SDRi.  ``pystoi`` is not installed in this image, so this is a from-scratch
fp64 restatement of the published algorithm as pystoi 0.3+ implements it:

* both signals are resampled to 10 kHz with the Octave-style polyphase filter
  (``resample_filter``; scipy.signal.resample_poly does the filtering);
* the clean signal is cut into Hann-windowed frames of 256 samples at hop 128; frames more
  than 40 dB below the loudest one are dropped from both signals, and both are rebuilt by
  overlap-add of the kept windowed frames;
* a 512-point STFT of the rebuilt signals, summed into 15 third-octave bands from 150 Hz
  (``thirdoct``), gives the band envelopes X, Y [15, Kk];
* every run of 30 consecutive frames is a segment.  STOI: the processed envelope is scaled to
  the clean one's energy per band, clipped at -15 dB signal-to-distortion, and correlated
  with the clean envelope per band; the score is the mean over bands and segments.  ESTOI:
  both envelopes are mean/variance-normalised along frames and then along bands, and the
  score is the mean over frames and segments of their inner product;
* fewer than 30 kept frames give 1e-5 (pystoi's value, which it returns with a warning).

Parity with pystoi is UNPINNED (pystoi is not installed and no fixture of its output
exists); tests/test_stoi_cpu.py checks the metric's defining properties instead (identity,
monotonicity in the SNR, scale invariance, the band table, the resampler against scipy, the
30-frame edge).

``stoi_device`` (below) computes both scores for a padded batch on the device
(csrc/ctn_stoi.hip through ctn_stoi_eval); ``stoi`` stays the host restatement
it is tested against (tests/test_gpu_stoi.py).
"""
from __future__ import annotations

import collections
import math

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUMBAND = 15
MINFREQ = 150
N = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = np.finfo(float).eps
TOO_SHORT = 1e-5                      # the score of fewer than N kept frames
WINDOW = np.hanning(N_FRAME + 2)[1:-1]
MAX_RATIO = 64                        # largest up or down of the library's resampler
MAX_HL = 4096

StoiDetails = collections.namedtuple("StoiDetails", "stoi estoi kept idx margin")


def thirdoct(fs=FS, nfft=NFFT, num_bands=NUMBAND, min_freq=MINFREQ):
    """-> (lo, hi): band b sums the rfft bins [lo[b], hi[b]); the edges are the bins nearest
    to min_freq * 2^((2b -+ 1) / 6) (pystoi's thirdoct)."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    freq_low = min_freq * np.power(2.0, (2 * k - 1) / 6)
    freq_high = min_freq * np.power(2.0, (2 * k + 1) / 6)
    lo = [int(np.argmin(np.square(f - fl))) for fl in freq_low]
    hi = [int(np.argmin(np.square(f - fh))) for fh in freq_high]
    return lo, hi


BAND_LO, BAND_HI = thirdoct()


def ratio(fs_sig):
    """-> (up, down), FS / fs_sig reduced."""
    fs_sig = int(fs_sig)
    if fs_sig < 1:
        raise ValueError(f"sample rate {fs_sig}")
    g = math.gcd(FS, fs_sig)
    return FS // g, fs_sig // g


def resample_filter(up, down):
    """-> (win [2 Hl + 1] with unit sum, Hl): the Octave-style low-pass of pystoi's
    resample_oct, 60 dB stop-band rejection, cut-off at 1 / (2 max(up, down))."""
    fc = 1.0 / (2 * max(up, down))
    Hl = int(np.ceil((60.0 - 8.0) / (28.714 * fc / 10.0)))
    t = np.arange(-Hl, Hl + 1)
    h = np.kaiser(2 * Hl + 1, 0.1102 * (60.0 - 8.7)) * (2 * up * fc * np.sinc(2 * fc * t))
    return h / np.sum(h), Hl


def resample_direct(x, up, down):
    """The polyphase index formula the device kernel evaluates:
    out[k] = sum_i hh[k down - i up + Hl] x[i], hh = up * win, i ascending inside the
    signal, k < ceil(len up / down).  Equals scipy.signal.resample_poly (test_stoi_cpu.py)."""
    x = np.asarray(x, dtype=np.float64)
    if up == down:
        return x.copy()
    win, Hl = resample_filter(up, down)
    hh = up * win
    n = -(-x.size * up // down)
    out = np.zeros(n)
    for k in range(n):
        i0 = max(0, -((Hl - k * down) // up))             # ceil((k down - Hl) / up)
        i1 = min(x.size - 1, (k * down + Hl) // up)
        acc = 0.0
        for i in range(i0, i1 + 1):
            acc += hh[k * down - i * up + Hl] * x[i]
        out[k] = acc
    return out


def resample(x, fs_sig):
    """x at fs_sig -> fp64 at FS (step 1)."""
    x = np.asarray(x, dtype=np.float64)
    up, down = ratio(fs_sig)
    if up == down:
        return x
    from scipy.signal import resample_poly
    return resample_poly(x, up, down, window=resample_filter(up, down)[0])


def _frames(s, starts):
    return np.stack([WINDOW * s[i:i + N_FRAME] for i in starts]) if len(starts) else np.zeros((0, N_FRAME))


def _keep(x):
    """-> (idx of the kept frames, margin in dB) from the clean signal alone (step 2)."""
    K = (x.size - N_FRAME) // HOP + 1 if x.size >= N_FRAME else 0
    if K == 0:
        return np.zeros(0, dtype=np.int64), np.inf
    e = 20.0 * np.log10(np.linalg.norm(_frames(x, range(0, HOP * K, HOP)), axis=1) + EPS)
    d = np.max(e) - DYN_RANGE - e
    return np.nonzero(d < 0)[0], float(np.min(np.abs(d)))


def _rebuild(s, idx):
    """Overlap-add of the kept windowed frames at hop 128, j ascending (step 3)."""
    z = np.zeros(HOP * (idx.size - 1) + N_FRAME)
    for j, k in enumerate(idx):
        z[HOP * j:HOP * j + N_FRAME] += WINDOW * s[HOP * k:HOP * k + N_FRAME]
    return z


def _bands(z, Kk):
    """-> [15, Kk]: square roots of the third-octave band sums of |STFT|^2 (step 4)."""
    spec = np.fft.rfft(_frames(z, range(0, HOP * Kk, HOP)), n=NFFT, axis=1)
    p = np.square(np.abs(spec))
    return np.sqrt(np.stack([p[:, lo:hi].sum(axis=1) for lo, hi in zip(BAND_LO, BAND_HI)]))


def _segments(X):
    return np.stack([X[:, s:s + N] for s in range(X.shape[1] - N + 1)])      # [J, 15, 30]


def _normalize(a, axis):
    a = a - np.mean(a, axis=axis, keepdims=True)
    return a / (np.linalg.norm(a, axis=axis, keepdims=True) + EPS)


def _scores(X, Y):
    xs, ys = _segments(X), _segments(Y)
    J = xs.shape[0]
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = np.minimum(ys * c, xs * (1.0 + 10.0 ** (-BETA / 20.0)))
    d = float(np.sum(_normalize(yp, 2) * _normalize(xs, 2)) / (NUMBAND * J))
    xn, yn = _normalize(_normalize(xs, 2), 1), _normalize(_normalize(ys, 2), 1)
    return d, float(np.sum(xn * yn / N) / J)


def stoi_details(x, y, fs_sig):
    """-> StoiDetails(stoi, estoi, kept, idx, margin): both scores, the number Kk and the
    numbers idx of the kept frames, and margin = min_k |max(e) - 40 - e_k| in dB, the
    distance of the nearest keep decision from its threshold."""
    x, y = np.asarray(x), np.asarray(y)
    if x.ndim != 1 or x.shape != y.shape:
        raise ValueError(f"x and y should be 1-D of equal length, got {x.shape} and {y.shape}")
    x, y = resample(x, fs_sig), resample(y, fs_sig)
    idx, margin = _keep(x)
    Kk = int(idx.size)
    if Kk < N:
        return StoiDetails(TOO_SHORT, TOO_SHORT, Kk, idx, margin)
    d, de = _scores(_bands(_rebuild(x, idx), Kk), _bands(_rebuild(y, idx), Kk))
    return StoiDetails(d, de, Kk, idx, margin)


def stoi(x, y, fs_sig, extended=False):
    """x clean, y processed, 1-D of equal length at fs_sig Hz -> STOI (ESTOI if extended);
    1e-5 when fewer than 30 frames survive the removal of silent frames."""
    r = stoi_details(x, y, fs_sig)
    return float(r.estoi if extended else r.stoi)


# ----------------------------------------------------------------------------
# Device path (csrc/ctn_stoi.hip through ctn_stoi_eval): the same chain for a ragged batch,
# every (signal, reference) pair of an utterance in one call.
# ----------------------------------------------------------------------------
WS_LIMIT = 1 << 30          # bytes of library workspace per call; larger batches are split
COMPACT_CHUNK = 256         # frames per step of the compaction kernel's prefix sum (STOI_CHUNK, ctn_stoi.h)
_tables = {}


def device_ratio(fs):
    """(up, down, Hl) of a sample rate the library's resampler supports, else ValueError."""
    up, down = ratio(fs)
    Hl = 0 if up == down else resample_filter(up, down)[1]
    if max(up, down) > MAX_RATIO or Hl > MAX_HL:
        raise ValueError(f"sample rate {fs}: the ratio {up}/{down} to {FS} Hz exceeds the device resampler's "
                         f"limit of {MAX_RATIO}")
    return up, down, Hl


def table(fs):
    """The fp64 table of ctn_stoi_eval: the window, (cos, -sin)(2 pi k / 512) for k < 256
    interleaved, and the resampling filter up * win (none for 1/1)."""
    up, down, _ = device_ratio(fs)
    k = np.arange(NFFT // 2)
    tw = np.stack((np.cos(2 * np.pi * k / NFFT), -np.sin(2 * np.pi * k / NFFT)), axis=1).reshape(-1)
    parts = [WINDOW, tw]
    if up != down:
        parts.append(up * resample_filter(up, down)[0])
    return np.concatenate(parts)


def _device_table(fs, device):
    import torch
    key = (int(fs), str(device))
    if key not in _tables:
        _tables[key] = torch.from_numpy(table(fs)).to(device)
    return _tables[key]


def stoi_device(refs, sigs, lengths=None, fs=8000):
    """refs [M, C, T], sigs [M, E, T] (device tensors at fs Hz; utterance m uses its first
    lengths[m] samples, the rest is never read) -> (stoi, estoi), each [M, E, C] fp64 on the
    device: the score of signal e against reference j, kept [M, C] the number of frames
    reference j keeps, and status [M, C] (1: fewer than 30, both scores are 1e-5)."""
    import ctypes

    import torch

    import ctn_lib as L
    from bss_eval import _lengths_tensor
    L.require_device(refs, "stoi_device")
    L.require_device(sigs, "stoi_device")
    if refs.dim() != 3 or sigs.dim() != 3 or refs.shape[0] != sigs.shape[0] or refs.shape[2] != sigs.shape[2]:
        raise ValueError(f"shape mismatch: references {tuple(refs.shape)}, signals {tuple(sigs.shape)}")
    up, down, Hl = device_ratio(fs)
    refs, sigs = refs.float().contiguous(), sigs.float().contiguous()
    (M, C, T), E = refs.shape, sigs.shape[1]
    lengths = _lengths_tensor(lengths, M, T, refs.device)
    tab = _device_table(fs, refs.device)
    lib = L.load()

    def desc(m):
        return L.StoiDesc(m, C, E, T, up, down, Hl)
    score = torch.empty(M, E, C, 2, dtype=torch.float64, device=refs.device)
    kept = torch.empty(M, C, dtype=torch.int32, device=refs.device)
    status = torch.empty(M, C, dtype=torch.int32, device=refs.device)
    one = lib.ctn_stoi_workspace_bytes(ctypes.byref(desc(1)))
    if one == 0:                  # unsupported shape: let the entry point name the reason
        L.check(lib.ctn_stoi_eval(ctypes.byref(desc(1)), None, None, None, None, None, None, None, None, 0, None),
                "ctn_stoi_eval")
    step = max(1, min(M, WS_LIMIT // one, 65535))
    ws = L.workspace(lib.ctn_stoi_workspace_bytes(ctypes.byref(desc(step))), refs.device)
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        L.check(lib.ctn_stoi_eval(ctypes.byref(desc(m1 - m0)), L.ptr(refs[m0:m1]), L.ptr(sigs[m0:m1]),
                                  L.ptr(lengths[m0:m1]), L.ptr(tab), L.ptr(score[m0:m1]), L.ptr(kept[m0:m1]),
                                  L.ptr(status[m0:m1]), L.ptr(ws), ws.numel(), L.stream_handle(refs.device)),
                "ctn_stoi_eval")
    return score[..., 0], score[..., 1], kept, status
