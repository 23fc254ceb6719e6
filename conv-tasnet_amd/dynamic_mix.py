"""Dynamic mixing: training batches drawn and mixed on the device.

The reference trains on the corpus's fixed mixtures, collated on the host
(src/data.py:131-159, 237-271).  Here the single-speaker utterances stay resident in
device memory (``DeviceCorpus``: 16-bit PCM as stored in the wav files, or fp32) and every
training batch is drawn (speaker-disjoint utterances, segment starts, levels) and mixed by
the HIP library (include/ctn.h: ctn_dmix_draw, ctn_dmix_mix) with no host work in the loop.

A batch row is a function of ``(seed, g)`` alone, g being the row's global sample number
``(step * world + rank) * M + m``: a run is reproducible, resumable, and independent of
how a global batch is split over ranks.

``philox4x32_10``, ``plan_host`` and ``mix_host`` restate the two device calls in numpy:
a batch can be reproduced on the host without a GPU (and the tests use them as the
reference).  ``mix_host`` computes its gains in fp64; given the gains a device call
reported it reproduces that call's sources and mixture bit for bit.

Speed perturbation (``DynamicMixer(..., speeds=(95, 100, 105))``): every
source is resampled on the device by a polyphase FIR before it is mixed
(ctn_dmix_draw_sp, ctn_dmix_mix_sp).  ``speed_ratio``, ``speed_filter``, ``segment_span``
and ``resample_host`` restate it, and ``plan_host`` / ``mix_host`` take ``speeds``.

Reverberation and noise (``DynamicMixer(..., rirs=RirBank(...), noise=corpus)``):
every source is optionally convolved on the device with a drawn room impulse response and the
mixture gets a drawn noise segment at a drawn SNR (ctn_dmix_draw_aug, ctn_dmix_mix_aug).
``reverb_host``, ``plan_aug_host`` and ``mix_aug_host`` restate them.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

PLAN_DTYPE = np.dtype([("utt", "<i4"), ("start", "<i4"), ("level_db", "<f4"), ("tries", "<i4")])
MAX_C, MAX_TRIES = 16, 64
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = 0xFFFFFFFF


# ----------------------------------------------------------------------------
# host restatement
# ----------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Random123): 4 counter words, 2 key words -> 4 output words."""
    c0, c1, c2, c3 = (int(c) & _U32 for c in counter)
    k0, k1 = (int(k) & _U32 for k in key)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _U32, (p0 >> 32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def eligible(off, T):
    """Indices (int32) of the utterances with at least T samples."""
    off = np.asarray(off, dtype=np.int64)
    return np.nonzero(np.diff(off) >= T)[0].astype(np.int32)


MAX_SPEEDS, MAX_RATIO = 8, 64


def speed_ratio(pct):
    """Speed in percent -> the reduced resampling ratio (up, down), output rate over input
    rate: up/down = 100/pct, so 95 -> (20, 19) and 105 -> (20, 21).  ValueError outside the
    library's limits (1 <= up, down <= 64, up <= 2 down, down <= 2 up)."""
    if isinstance(pct, bool) or int(pct) != pct or int(pct) < 1:
        raise ValueError(f"speed {pct!r}: a positive integer percent")
    g = np.gcd(100, int(pct))
    up, down = 100 // int(g), int(pct) // int(g)
    if up > MAX_RATIO or down > MAX_RATIO or up > 2 * down or down > 2 * up:
        raise ValueError(f"speed {pct} % is the ratio {up}/{down}: outside the limits (up, down <= {MAX_RATIO}, "
                         f"between 1/2 and 2)")
    return up, down


def _speed_filter64(up, down):
    hl = 10 * max(up, down)
    n = np.arange(-hl, hl + 1, dtype=np.float64)
    fc = 1.0 / max(up, down)
    h = fc * np.sinc(fc * n) * np.kaiser(2 * hl + 1, 5.0)
    return h / h.sum() * up, hl


def speed_filter(up, down):
    """(h float32 [2 Hl + 1], Hl): the filter of scipy.signal.resample_poly(x, up, down) —
    Hl = 10 max(up, down), a sinc of cut-off 1/max(up, down) under a Kaiser window (beta 5),
    unit sum, times up; computed in fp64 and rounded once."""
    h, hl = _speed_filter64(up, down)
    return h.astype(np.float32), hl


def segment_span(T, up, down):
    """Input samples under the centres of T outputs: floor((T - 1) down / up) + 1."""
    return (int(T) - 1) * int(down) // int(up) + 1


def resample_host(wave_f32, start, T, up, down):
    """The resampled segment of ctn_dmix_mix_sp: xr[n] = sum_i h[n down - i up + Hl] x[i],
    x[i] = wave[start + i], for n = 0 ... T - 1; i upward, acc = fl32(acc + fl32(h x)) from 0;
    terms whose x lies outside the wave are skipped.  1/1: the samples themselves."""
    x = np.asarray(wave_f32, np.float32)
    n = np.arange(T, dtype=np.int64)
    if len(x) == 0:
        return np.zeros(T, np.float32)
    if (up, down) == (1, 1):
        a = int(start) + n
        ok = (a >= 0) & (a < len(x))
        out = np.zeros(T, np.float32)
        out[ok] = x[a[ok]]
        return out
    h, hl = speed_filter(up, down)
    t = n * down + hl
    q, p = t // up, t % up
    acc = np.zeros(T, np.float32)
    for j in range(2 * hl // up, -1, -1):                # i = q - j runs upward
        hi, a = p + j * up, int(start) + q - j
        ok = (hi <= 2 * hl) & (a >= 0) & (a < len(x))
        term = h[np.where(ok, hi, 0)] * x[np.where(ok, a, 0)]        # fp32 product, one rounding
        acc = np.where(ok, acc + term, acc)
    return acc


def _speed_table(speeds):
    """Percents -> [(up, down)] (1 to 8 entries)."""
    ratios = [speed_ratio(p) for p in speeds]
    if not 1 <= len(ratios) <= MAX_SPEEDS:
        raise ValueError(f"{len(ratios)} speeds: 1 to {MAX_SPEEDS}")
    return ratios


def plan_host(off, spk, elig, M, C, T, seed=0, first_sample=0, level_db=(-2.5, 2.5), max_tries=16, speeds=None):
    """The plan ctn_dmix_draw writes: a [M, C] array of PLAN_DTYPE.  With `speeds` (percents):
    (plan, speed_idx [M, C] int32) as ctn_dmix_draw_sp writes them; `elig` should then hold
    the utterances of at least max_k segment_span(T, up_k, down_k) samples."""
    off, spk, elig = np.asarray(off, np.int64), np.asarray(spk, np.int32), np.asarray(elig, np.int32)
    U, E = len(spk), len(elig)
    lo, hi = np.float32(level_db[0]), np.float32(level_db[1])
    key = (int(seed) & _U32, (int(seed) >> 32) & _U32)
    plan = np.zeros((M, C), dtype=PLAN_DTYPE)
    spans = [T] if speeds is None else [segment_span(T, up, down) for up, down in _speed_table(speeds)]
    speed_idx = np.zeros((M, C), np.int32)
    for m in range(M):
        g = (int(first_sample) + m) & 0xFFFFFFFFFFFFFFFF
        taken = []                                       # speakers of the accepted valid slots
        for c in range(C):
            for j in range(max_tries):
                r = philox4x32_10((g & _U32, g >> 32, c, j), key)
                k = (r[3] * len(spans)) >> 32
                utt = int(elig[(r[0] * E) >> 32])
                level = lo + (hi - lo) * (np.float32(r[2] >> 8) * np.float32(2.0 ** -24))
                e = (-1, 0, level, j + 1)
                n = int(off[utt + 1] - off[utt]) - spans[k] + 1 if 0 <= utt < U else 0
                if n < 1 or n > 0x7FFFFFFF:
                    sp = None
                    break
                e = (utt, (r[1] * n) >> 32, level, j + 1)
                sp = int(spk[utt])
                if sp not in taken:
                    break
            plan[m, c] = e
            speed_idx[m, c] = k
            if sp is not None and e[0] >= 0:
                taken.append(sp)
    return plan if speeds is None else (plan, speed_idx)


def _segment(pool, off, e, T, ratios=None, k=0):
    """fp32 samples of a plan entry (resampled at ratios[k] when given), or None for an
    entry that must not be read."""
    U = len(off) - 1
    utt, start = int(e["utt"]), int(e["start"])
    if ratios is not None and not 0 <= k < len(ratios):
        return None
    up, down = (1, 1) if ratios is None else ratios[k]
    if not 0 <= utt < U or start < 0 or start + segment_span(T, up, down) > int(off[utt + 1] - off[utt]):
        return None
    if (up, down) != (1, 1):
        x = pool[int(off[utt]):int(off[utt + 1])]
        x = x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x.astype(np.float32, copy=False)
        return resample_host(x, start, T, up, down)
    x = pool[int(off[utt]) + start:int(off[utt]) + start + T]
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(2.0 ** -15)
    return x.astype(np.float32, copy=False)


def mix_host(pool, off, plan, T, level_mode=0, peak=0.9, gains=None, speeds=None, speed_idx=None):
    """ctn_dmix_mix on the host.  pool: int16 or float32 [n]; plan: [M, C] PLAN_DTYPE.
    With `speeds` (percents) and `speed_idx` [M, C]: ctn_dmix_mix_sp, every segment resampled
    (resample_host) before the level, RMS and peak stages.

    -> dict(gains [M, C] float64: the gains in fp64 arithmetic; p [M] float64: the
    unguarded mixture's peak; sources [M, C, T], mixture [M, T] float32; status [M] int32).
    sources and mixture follow the exactness contract with the fp32 gains `gains` when
    given (a device call's read-back gains), else with the fp64 gains rounded to fp32."""
    off = np.asarray(off, np.int64)
    M, C = plan.shape
    g64, p64 = np.zeros((M, C)), np.zeros(M)
    sources, mixture = np.zeros((M, C, T), np.float32), np.zeros((M, T), np.float32)
    status = np.zeros(M, np.int32)
    ratios = None if speeds is None else _speed_table(speeds)
    if ratios is not None and (speed_idx is None or np.shape(speed_idx) != (M, C)):
        raise ValueError(f"speeds need speed_idx of shape {(M, C)}")
    for m in range(M):
        xs = [_segment(pool, off, plan[m, c], T, ratios, 0 if ratios is None else int(speed_idx[m, c]))
              for c in range(C)]
        if any(x is None for x in xs):
            status[m] = 1
            continue
        for c, x in enumerate(xs):
            g = 10.0 ** (float(plan[m, c]["level_db"]) / 20.0)
            if level_mode == 1:
                g /= max(float(np.sqrt(np.mean(x.astype(np.float64) ** 2))), 1e-4)
            g64[m, c] = g
        p64[m] = np.abs(sum(g64[m, c] * xs[c].astype(np.float64) for c in range(C))).max()
        if peak > 0 and p64[m] > peak:
            g64[m] *= peak / p64[m]
        g32 = g64[m].astype(np.float32) if gains is None else np.asarray(gains, np.float32)[m]
        for c, x in enumerate(xs):
            sources[m, c] = g32[c] * x                     # one fp32 rounding per sample
            mixture[m] = sources[m, c] if c == 0 else mixture[m] + sources[m, c]
    return {"gains": g64, "p": p64, "sources": sources, "mixture": mixture, "status": status}


MAX_RIR_TAPS = 16384
_RIR_SLOT, _NOISE_SLOT = 16, 32                          # Philox counter word 2 of the RIR and noise draws


_COUNT_SLOT = 48                                         # Philox counter word 2 of the speaker-count draw


def thin_host(plan, M, C, seed, first_sample, min_speakers):
    """ctn_dmix_thin on the host -> (plan, count [M] int32): a copy of `plan` in which row m keeps
    its first n_m = min_speakers + ((r0 (C - min_speakers + 1)) >> 32) slots and the others have
    level_db = -inf (a gain of exactly 0 in mix_host / mix_aug_host); r0 is word 0 of the row's
    own draw at counter word 2 = 48, so the count depends on (seed, global sample) alone."""
    if not 1 <= int(min_speakers) <= C:
        raise ValueError(f"min_speakers={min_speakers} outside 1..C={C}")
    plan = np.array(plan, dtype=PLAN_DTYPE, copy=True).reshape(M, C)
    key = (int(seed) & _U32, (int(seed) >> 32) & _U32)
    count = np.zeros(M, np.int32)
    for m in range(M):
        g = (int(first_sample) + m) & 0xFFFFFFFFFFFFFFFF
        r = philox4x32_10((g & _U32, g >> 32, _COUNT_SLOT, 0), key)
        count[m] = int(min_speakers) + ((r[0] * (C - int(min_speakers) + 1)) >> 32)
        plan["level_db"][m, count[m]:] = -np.inf
    return plan, count


def reverb_host(xs, h):
    """The reverberated segment of ctn_dmix_mix_aug: xv[n] = sum_{j <= min(n, L - 1)} h[j] xs[n - j],
    j upward, acc = fl32(acc + fl32(h[j] xs[n - j])) from +0; the segment starts from silence."""
    xs, h = np.asarray(xs, np.float32), np.asarray(h, np.float32)
    T = len(xs)
    acc = np.zeros(T, np.float32)
    for j in range(min(T, len(h))):
        acc[j:] = acc[j:] + h[j] * xs[:T - j]            # fp32 product, one rounding; then the sum
    return acc


def plan_aug_host(off, spk, elig, M, C, T, seed=0, first_sample=0, level_db=(-2.5, 2.5), max_tries=16, speeds=None,
                  n_rirs=0, rir_prob=1.0, noise_off=None, noise_elig=None, snr_db=(-5.0, 5.0)):
    """What ctn_dmix_draw_aug writes -> dict(plan [M, C] PLAN_DTYPE, speed_idx [M, C] int32 (zeros
    without speeds), rir [M, C] int32, nplan [M] PLAN_DTYPE or None without a noise pool)."""
    src = plan_host(off, spk, elig, M, C, T, seed=seed, first_sample=first_sample, level_db=level_db,
                    max_tries=max_tries, speeds=speeds)
    plan, speed_idx = (src, np.zeros((M, C), np.int32)) if speeds is None else src
    key = (int(seed) & _U32, (int(seed) >> 32) & _U32)
    prob, two24 = np.float32(rir_prob), np.float32(2.0 ** -24)
    rir = np.full((M, C), -1, np.int32)
    nplan = None
    if noise_off is not None:
        noise_off, noise_elig = np.asarray(noise_off, np.int64), np.asarray(noise_elig, np.int32)
        nplan = np.zeros(M, dtype=PLAN_DTYPE)
        lo, hi = np.float32(snr_db[0]), np.float32(snr_db[1])
    for m in range(M):
        g = (int(first_sample) + m) & 0xFFFFFFFFFFFFFFFF
        for c in range(C):
            r = philox4x32_10((g & _U32, g >> 32, _RIR_SLOT + c, 0), key)
            if n_rirs > 0 and np.float32(r[1] >> 8) * two24 < prob:
                rir[m, c] = (r[0] * n_rirs) >> 32
        if nplan is not None:
            r = philox4x32_10((g & _U32, g >> 32, _NOISE_SLOT, 0), key)
            utt = int(noise_elig[(r[0] * len(noise_elig)) >> 32])
            snr = lo + (hi - lo) * (np.float32(r[2] >> 8) * two24)
            n = int(noise_off[utt + 1] - noise_off[utt]) - T + 1 if 0 <= utt < len(noise_off) - 1 else 0
            nplan[m] = (utt, (r[1] * n) >> 32, snr, 1) if 1 <= n <= 0x7FFFFFFF else (-1, 0, snr, 1)
    return {"plan": plan, "speed_idx": speed_idx, "rir": rir, "nplan": nplan}


def mix_aug_host(pool, off, plan, T, level_mode=0, peak=0.9, gains=None, ngain=None, speeds=None, speed_idx=None,
                 rirs=None, rir=None, noise_pool=None, noise_off=None, nplan=None):
    """ctn_dmix_mix_aug on the host.  rirs: list of fp32 tap arrays with rir [M, C] int32 (-1: dry);
    noise_pool / noise_off / nplan [M] PLAN_DTYPE (level_db = snr_db): the noise stage.

    -> dict(gains [M, C], ngain [M] float64: the gains in fp64 arithmetic; p [M] float64: the
    unguarded mixture's peak; sources [M, C, T], mixture [M, T], noise [M, T] float32; status).
    sources, mixture and noise follow the exactness contract with the fp32 `gains` / `ngain`
    when given (a device call's read-back), else with the fp64 gains rounded to fp32."""
    off = np.asarray(off, np.int64)
    M, C = plan.shape
    g64, n64, p64 = np.zeros((M, C)), np.zeros(M), np.zeros(M)
    sources, mixture = np.zeros((M, C, T), np.float32), np.zeros((M, T), np.float32)
    noise = np.zeros((M, T), np.float32)
    status = np.zeros(M, np.int32)
    ratios = None if speeds is None else _speed_table(speeds)
    if ratios is not None and (speed_idx is None or np.shape(speed_idx) != (M, C)):
        raise ValueError(f"speeds need speed_idx of shape {(M, C)}")
    if rirs is not None and (rir is None or np.shape(rir) != (M, C)):
        raise ValueError(f"rirs need rir of shape {(M, C)}")
    if noise_pool is not None and (nplan is None or np.shape(nplan) != (M,)):
        raise ValueError(f"a noise pool needs nplan of shape {(M,)}")
    for m in range(M):
        xs = [_segment(pool, off, plan[m, c], T, ratios, 0 if ratios is None else int(speed_idx[m, c]))
              for c in range(C)]
        z = None if noise_pool is None else _segment(noise_pool, np.asarray(noise_off, np.int64), nplan[m], T)
        bad = any(x is None for x in xs) or (noise_pool is not None and z is None)
        if rirs is not None:
            ks = [int(k) for k in rir[m]]
            bad = bad or any(not -1 <= k < len(rirs) or (k >= 0 and not 1 <= len(rirs[k]) <= MAX_RIR_TAPS) for k in ks)
        if bad:
            status[m] = 1
            continue
        if rirs is not None:
            xs = [x if k < 0 else reverb_host(x, rirs[k]) for x, k in zip(xs, ks)]
        for c, x in enumerate(xs):
            g = 10.0 ** (float(plan[m, c]["level_db"]) / 20.0)
            if level_mode == 1:
                g /= max(float(np.sqrt(np.mean(x.astype(np.float64) ** 2))), 1e-4)
            g64[m, c] = g
        clean = sum(g64[m, c] * xs[c].astype(np.float64) for c in range(C))
        if z is not None:
            s = None                                     # the fp32 mixture before the guard, fp32 gains
            for c, x in enumerate(xs):
                v = np.float32(g64[m, c]) * x
                s = v if s is None else s + v
            ps, pz = np.mean(s.astype(np.float64) ** 2), np.mean(z.astype(np.float64) ** 2)
            n64[m] = np.sqrt(ps / max(pz, 1e-8)) * 10.0 ** (-float(nplan[m]["level_db"]) / 20.0)
            clean = clean + n64[m] * z.astype(np.float64)
        p64[m] = np.abs(clean).max()
        if peak > 0 and p64[m] > peak:
            g64[m] *= peak / p64[m]
            n64[m] *= peak / p64[m]
        g32 = g64[m].astype(np.float32) if gains is None else np.asarray(gains, np.float32)[m]
        for c, x in enumerate(xs):
            sources[m, c] = g32[c] * x                     # one fp32 rounding per sample
            mixture[m] = sources[m, c] if c == 0 else mixture[m] + sources[m, c]
        if z is not None:
            noise[m] = (np.float32(n64[m]) if ngain is None else np.asarray(ngain, np.float32)[m]) * z
            mixture[m] = mixture[m] + noise[m]
    return {"gains": g64, "ngain": n64, "p": p64, "sources": sources, "mixture": mixture, "noise": noise,
            "status": status}


# ----------------------------------------------------------------------------
# device side
# ----------------------------------------------------------------------------
def wsj0_speaker_of(path, slot):
    """wsj0-2mix: `<utt1>_<snr1>_<utt2>_<snr2>.wav`; the speaker of slot c is the first three
    characters of field 2 (c - 1).  A name that does not parse is its own speaker."""
    fields = os.path.splitext(os.path.basename(path))[0].split("_")
    i = 2 * (slot - 1)
    if len(fields) < 2 * slot or len(fields[i]) < 3:
        return ("file", path, slot)
    return fields[i][:3]


class DeviceCorpus:
    """Single-speaker utterances resident in device memory, back to back.

    waves: numpy arrays [n_i], int16 (PCM: value s * 2^-15) or floating; the pool is int16
    when every one is int16, else fp32.  speakers: one hashable label per utterance."""

    def __init__(self, waves, speakers, device):
        import torch
        if len(waves) == 0 or len(waves) != len(speakers):
            raise ValueError(f"{len(waves)} utterances with {len(speakers)} speaker labels")
        waves = [np.asarray(w).reshape(-1) for w in waves]
        pcm = all(w.dtype == np.int16 for w in waves)
        if not pcm:
            waves = [w.astype(np.float32) * np.float32(2.0 ** -15) if w.dtype == np.int16 else w.astype(np.float32)
                     for w in waves]
        self.pool_dtype = 0 if pcm else 1
        self.off_host = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
        ids = {}
        self.spk_host = np.array([ids.setdefault(s, len(ids)) for s in speakers], dtype=np.int32)
        self.speaker_labels = list(ids)
        self.device = torch.device(device)
        pool = np.concatenate(waves) if self.off_host[-1] > 0 else np.zeros(1, np.int16 if pcm else np.float32)
        self.pool = torch.from_numpy(pool).to(self.device)
        self.off = torch.from_numpy(self.off_host).to(self.device)
        self.spk = torch.from_numpy(self.spk_host).to(self.device)
        self._elig = {}

    @property
    def n_utts(self):
        return len(self.spk_host)

    @property
    def nbytes(self):
        """Bytes of device memory the corpus holds (pool and tables)."""
        return sum(t.numel() * t.element_size() for t in (self.pool, self.off, self.spk))

    def eligible(self, T, C=1):
        """(device int32 tensor, host array) of the utterances of at least T samples;
        ValueError when they have fewer than C distinct speakers."""
        import torch
        if T not in self._elig:
            host = eligible(self.off_host, T)
            self._elig[T] = (torch.from_numpy(host).to(self.device), host)
        dev, host = self._elig[T]
        nspk = len(set(self.spk_host[host].tolist()))
        if len(host) == 0 or nspk < C:
            raise ValueError(f"dynamic mixing of {C} speakers needs {C} distinct speakers among the utterances of "
                             f"at least {T} samples; the corpus has {len(host)} such utterances from {nspk} speakers")
        return dev, host

    @classmethod
    def from_json_dir(cls, json_dir, sample_rate, speaker_of=None, max_bytes=64 << 30, device="cuda"):
        """Every utterance of s1.json ... sC.json (lists of [wav_path, #samples]).  int16 when
        every file is mono 16-bit PCM at sample_rate, else fp32 as audio_io.read_wav returns."""
        import json

        import audio_io
        from data import speaker_names
        speaker_of = speaker_of or wsj0_speaker_of
        waves, speakers, samples, pcm = [], [], 0, True
        for slot, name in enumerate(speaker_names(json_dir), start=1):
            with open(os.path.join(json_dir, name + ".json")) as f:
                infos = json.load(f)
            for path, _ in infos:
                (tag, ch, rate, align, bits), payload = audio_io._read(path)
                if tag == audio_io.WAVE_FORMAT_PCM and bits == 16 and ch == 1 and rate == int(sample_rate):
                    w = np.frombuffer(payload[:len(payload) // 2 * 2], "<i2").astype(np.int16)
                else:
                    w, pcm = audio_io.read_wav(path, sr=sample_rate)[0], False
                samples += len(w)
                if samples * (2 if pcm else 4) > max_bytes:
                    raise ValueError(f"{json_dir}: the source utterances need more than max_bytes={max_bytes} "
                                     f"of device memory (reached at {path})")
                waves.append(w)
                speakers.append(speaker_of(path, slot))
        return cls(waves, speakers, device)

    @classmethod
    def from_wav_dir(cls, wav_dir, sample_rate, device="cuda"):
        """Every *.wav of wav_dir (sorted) as one utterance each, e.g. a noise pool; fp32 as
        audio_io.read_wav returns, every file its own speaker."""
        import audio_io
        names = sorted(n for n in os.listdir(wav_dir) if n.lower().endswith(".wav"))
        if not names:
            raise ValueError(f"{wav_dir}: no wav files")
        return cls([audio_io.read_wav(os.path.join(wav_dir, n), sr=sample_rate)[0] for n in names], names, device)


def plan_to_numpy(plan):
    """Device plan tensor (int32 [M, C, 4]) -> [M, C] array of PLAN_DTYPE."""
    a = plan.detach().cpu().numpy()
    return a.view(PLAN_DTYPE).reshape(a.shape[0], a.shape[1])


def plan_from_numpy(plan, device):
    import torch
    a = np.ascontiguousarray(plan, dtype=PLAN_DTYPE)
    return torch.from_numpy(a.view(np.int32).reshape(a.shape[0], a.shape[1], 4).copy()).to(device)


class RirBank:
    """Room impulse responses resident in device memory, fp32 taps back to back.

    rirs: arrays [L_i]; max_taps truncates the longer ones.  ValueError for an empty RIR or one of
    more than 16384 taps (after truncation)."""

    def __init__(self, rirs, device, max_taps=None):
        import torch
        rirs = [np.asarray(h, np.float32).reshape(-1) for h in rirs]
        if max_taps is not None:
            if int(max_taps) < 1:
                raise ValueError(f"max_taps={max_taps}")
            rirs = [h[:int(max_taps)] for h in rirs]
        if len(rirs) == 0:
            raise ValueError("no room impulse responses")
        for i, h in enumerate(rirs):
            if not 1 <= len(h) <= MAX_RIR_TAPS:
                raise ValueError(f"room impulse response {i} has {len(h)} taps: 1 to {MAX_RIR_TAPS}")
        self.rirs_host = rirs
        self.roff_host = np.concatenate([[0], np.cumsum([len(h) for h in rirs])]).astype(np.int64)
        self.max_len = max(len(h) for h in rirs)
        self.device = torch.device(device)
        self.pool = torch.from_numpy(np.concatenate(rirs)).to(self.device)
        self.roff = torch.from_numpy(self.roff_host).to(self.device)

    def __len__(self):
        return len(self.rirs_host)

    @classmethod
    def from_dir(cls, rir_dir, sample_rate, max_taps=MAX_RIR_TAPS, device="cuda"):
        """Every *.wav of rir_dir (sorted), mono through audio_io.read_wav at sample_rate;
        `truncated` counts the files that had more than max_taps samples."""
        import audio_io
        names = sorted(n for n in os.listdir(rir_dir) if n.lower().endswith(".wav"))
        if not names:
            raise ValueError(f"{rir_dir}: no wav files")
        rirs = [audio_io.read_wav(os.path.join(rir_dir, n), sr=sample_rate)[0] for n in names]
        bank = cls(rirs, device, max_taps=max_taps)
        bank.truncated = sum(len(h) > int(max_taps) for h in rirs)
        return bank


class DynamicMixer:
    """Draws and mixes batches of M rows, C speakers, T samples on the corpus's device.

    level_mode 0: gain 10^(level_db / 20) on the stored waveform; 1: relative to the
    segment's RMS (floored at 1e-4).  level_db: (lo, hi) of the uniform level draw.
    peak > 0: a row whose mixture would exceed it is scaled down to it.
    speeds: integer percents, e.g. (95, 100, 105): every source is played at one of them,
    drawn per slot, through the library's polyphase resampler (ctn_dmix_draw_sp,
    ctn_dmix_mix_sp; `.speed` holds the drawn indices).  None or all 100: no resampling, the
    plain entry points.
    rirs: a RirBank: every slot is convolved with one of its responses with probability rir_prob
    (`.rir` holds the drawn indices, -1: dry).  noise: a DeviceCorpus: every row gets one of its
    segments at an SNR drawn from snr_db = (lo, hi) (`.nplan`, `.ngain`).  Either one selects
    ctn_dmix_draw_aug / ctn_dmix_mix_aug; both None: the entry points above.
    min_speakers: 1 <= K < C: every row keeps a drawn number n_m in [K, C] of its slots
    (ctn_dmix_thin after the draw; `.count` holds n_m) and the others are silent: their
    level_db is -inf, their gain and every sample of their source exactly 0.  None or C: every
    slot speaks and no further kernel runs."""

    def __init__(self, corpus, M, C, T, seed=0, level_mode=0, level_db=(-2.5, 2.5), peak=0.9, max_tries=16,
                 rank=0, world=1, speeds=None, rirs=None, rir_prob=1.0, noise=None, snr_db=(-5.0, 5.0),
                 min_speakers=None):
        import torch

        import ctn_lib as L
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world size {world}")
        L.require_device(corpus.pool, "DynamicMixer")
        self.corpus, self.M, self.C, self.T = corpus, int(M), int(C), int(T)
        self.rank, self.world = int(rank), int(world)
        if min_speakers is not None and not 1 <= int(min_speakers) <= self.C:
            raise ValueError(f"min_speakers={min_speakers} outside 1..C={self.C}")
        self.min_speakers = None if min_speakers is None or int(min_speakers) == self.C else int(min_speakers)
        ratios = None if speeds is None else _speed_table(speeds)
        if ratios is not None and all(r == (1, 1) for r in ratios):
            ratios = None
        self.speeds = None if ratios is None else tuple(int(p) for p in speeds)
        self.ratios = ratios
        need = self.T if ratios is None else max(segment_span(self.T, up, down) for up, down in ratios)
        self.elig, self.elig_host = corpus.eligible(need, self.C)
        self.desc = L.DmixDesc(M=self.M, C=self.C, T=self.T, n_utts=corpus.n_utts, n_elig=len(self.elig_host),
                               pool_dtype=corpus.pool_dtype, level_mode=int(level_mode), max_tries=int(max_tries),
                               level_lo_db=float(level_db[0]), level_hi_db=float(level_db[1]), peak=float(peak),
                               seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._lib = L.load()
        self.speed = self._filt = self._sp = None
        self.rirs, self.noise, self._aug = rirs, noise, None
        self.rir = self.nplan = self.ngain = self.nelig = self.nelig_host = None
        if ratios is not None:
            self._sp = L.DmixSpeeds(n=len(ratios))
            for k, (up, down) in enumerate(ratios):
                self._sp.r[k].up, self._sp.r[k].down = up, down
        if rirs is not None or noise is not None:
            for what, other in (("rirs", rirs), ("noise", noise)):
                if other is not None and other.pool.device != corpus.pool.device:
                    raise ValueError(f"{what}: on {other.pool.device}, the corpus is on {corpus.pool.device}")
            self._aug = L.DmixAug(rir_prob=float(rir_prob), snr_lo_db=float(snr_db[0]), snr_hi_db=float(snr_db[1]))
            if rirs is not None:
                self._aug.n_rirs, self._aug.rir_max_taps = len(rirs), rirs.max_len
            if noise is not None:
                if len(eligible(noise.off_host, self.T)) == 0:
                    raise ValueError(f"noise: no recording holds the {self.T} samples of a segment")
                self.nelig, self.nelig_host = noise.eligible(self.T, 0)
                self._aug.n_noise_utts, self._aug.n_noise_elig = noise.n_utts, len(self.nelig_host)
                self._aug.noise_dtype = noise.pool_dtype
            nbytes = self._lib.ctn_dmix_aug_workspace_bytes(ctypes.byref(self.desc), self._sp_ref(),
                                                            ctypes.byref(self._aug))
            if nbytes == 0:                              # raises with the library's reason
                L.check(self._lib.ctn_dmix_draw_aug(ctypes.byref(self.desc), self._sp_ref(), ctypes.byref(self._aug),
                                                    None, None, None, None, None, 0, None, 0, None, None, None, None,
                                                    None), "DynamicMixer")
        elif ratios is None:
            nbytes = self._lib.ctn_dmix_workspace_bytes(ctypes.byref(self.desc))
        else:
            nbytes = self._lib.ctn_dmix_sp_workspace_bytes(ctypes.byref(self.desc), ctypes.byref(self._sp))
            if nbytes == 0:                              # raises with the library's reason
                L.check(self._lib.ctn_dmix_draw_sp(ctypes.byref(self.desc), ctypes.byref(self._sp), None, None, None,
                                                   0, None, 0, None, None, None), "DynamicMixer")
        if nbytes == 0:
            L.check(self._lib.ctn_dmix_draw(ctypes.byref(self.desc), None, None, None, 0, None, 0, None, None),
                    "DynamicMixer")                     # raises with the library's reason
        dev = corpus.device
        self._ws = L.workspace(nbytes, dev)
        self.plan = torch.zeros(self.M, self.C, 4, dtype=torch.int32, device=dev)
        self.gains = torch.zeros(self.M, self.C, dtype=torch.float32, device=dev)
        self.status = torch.zeros(self.M, dtype=torch.int32, device=dev)
        self.lengths = torch.full((self.M,), self.T, dtype=torch.int64, device=dev)
        self.count = torch.full((self.M,), self.C, dtype=torch.int32, device=dev)
        if ratios is not None:
            taps = np.concatenate([speed_filter(up, down)[0] for up, down in ratios if (up, down) != (1, 1)])
            if len(taps) != self._lib.ctn_dmix_sp_filter_floats(ctypes.byref(self._sp)):
                raise L.CtnLibraryError(f"filter table of {len(taps)} taps, the library expects "
                                        f"{self._lib.ctn_dmix_sp_filter_floats(ctypes.byref(self._sp))}")
            self._filt = torch.from_numpy(taps).to(dev)
            self.speed = torch.zeros(self.M, self.C, dtype=torch.int32, device=dev)
        if self._aug is not None:
            self.rir = torch.full((self.M, self.C), -1, dtype=torch.int32, device=dev)
            self.ngain = torch.zeros(self.M, dtype=torch.float32, device=dev)
            if noise is not None:
                self.nplan = torch.zeros(self.M, 1, 4, dtype=torch.int32, device=dev)

    def _sp_ref(self):
        return None if self._sp is None else ctypes.byref(self._sp)

    def first_sample(self, step):
        return (int(step) * self.world + self.rank) * self.M

    def _checked(self, t, what, dtype, shape):
        """The library trusts its pointers: a caller's tensor must be exactly what it expects."""
        if (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                or t.device != self.corpus.pool.device):
            raise ValueError(f"{what}: expected a contiguous {dtype} tensor of shape {shape} on "
                             f"{self.corpus.pool.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t

    def draw(self, first_sample=0, counter=None, advance=0):
        """Fill self.plan for the rows first_sample + m, or *counter + m (a device int64
        tensor of one element, to which `advance` is then added on the device).  With
        min_speakers the plan is then thinned and self.count filled."""
        import ctn_lib as L
        self._draw(first_sample, counter, advance)
        if self.min_speakers is not None:
            L.check(self._lib.ctn_dmix_thin(ctypes.byref(self.desc), self.min_speakers, int(first_sample),
                                            L.ptr(counter), int(advance), L.ptr(self.plan), L.ptr(self.count),
                                            L.stream_handle(self.corpus.device)), "ctn_dmix_thin")
        return self.plan

    def _draw(self, first_sample, counter, advance):
        import torch

        import ctn_lib as L
        c = self.corpus
        if counter is not None:
            self._checked(counter, "counter", torch.int64, (1,))
        if self._aug is not None:
            n = self.noise
            L.check(self._lib.ctn_dmix_draw_aug(ctypes.byref(self.desc), self._sp_ref(), ctypes.byref(self._aug),
                                                L.ptr(c.off), L.ptr(c.spk), L.ptr(self.elig),
                                                None if n is None else L.ptr(n.off), L.ptr(self.nelig),
                                                int(first_sample), L.ptr(counter), int(advance), L.ptr(self.plan),
                                                L.ptr(self.speed), L.ptr(self.rir), L.ptr(self.nplan),
                                                L.stream_handle(c.device)), "ctn_dmix_draw_aug")
            return self.plan
        if self.ratios is not None:
            L.check(self._lib.ctn_dmix_draw_sp(ctypes.byref(self.desc), ctypes.byref(self._sp), L.ptr(c.off),
                                               L.ptr(c.spk), L.ptr(self.elig), int(first_sample), L.ptr(counter),
                                               int(advance), L.ptr(self.plan), L.ptr(self.speed),
                                               L.stream_handle(c.device)), "ctn_dmix_draw_sp")
            return self.plan
        L.check(self._lib.ctn_dmix_draw(ctypes.byref(self.desc), L.ptr(c.off), L.ptr(c.spk), L.ptr(self.elig),
                                        int(first_sample), L.ptr(counter), int(advance), L.ptr(self.plan),
                                        L.stream_handle(c.device)), "ctn_dmix_draw")
        return self.plan

    def mix(self, plan=None, sources=None, mixture=None, speed=None, rir=None, nplan=None, noise_out=None):
        """Mix `plan` (default: the last drawn) -> (mixture [M, T], sources [M, C, T]).
        speed: with speeds, the int32 [M, C] speed indices of `plan` (default: the last drawn).
        rir: with rirs, the int32 [M, C] RIR indices (-1: dry); nplan: with noise, the int32
        [M, 1, 4] noise plan (plan_from_numpy of [M, 1] entries); noise_out: with noise, a float32
        [M, T] tensor that receives the scaled noise."""
        import torch

        import ctn_lib as L
        c = self.corpus
        if plan is not None:
            self.plan = self._checked(plan, "plan", torch.int32, (self.M, self.C, 4))
        if speed is not None:
            if self.ratios is None:
                raise ValueError("speed: this mixer was built without speeds")
            self.speed = self._checked(speed, "speed", torch.int32, (self.M, self.C))
        if sources is None:
            sources = torch.empty(self.M, self.C, self.T, dtype=torch.float32, device=c.device)
        if mixture is None:
            mixture = torch.empty(self.M, self.T, dtype=torch.float32, device=c.device)
        self._checked(sources, "sources", torch.float32, (self.M, self.C, self.T))
        self._checked(mixture, "mixture", torch.float32, (self.M, self.T))
        if rir is not None:
            if self.rirs is None:
                raise ValueError("rir: this mixer was built without rirs")
            self.rir = self._checked(rir, "rir", torch.int32, (self.M, self.C))
        if nplan is not None or noise_out is not None:
            if self.noise is None:
                raise ValueError("nplan, noise_out: this mixer was built without noise")
            if nplan is not None:
                self.nplan = self._checked(nplan, "nplan", torch.int32, (self.M, 1, 4))
            if noise_out is not None:
                self._checked(noise_out, "noise_out", torch.float32, (self.M, self.T))
        if self._aug is not None:
            b, n = self.rirs, self.noise
            L.check(self._lib.ctn_dmix_mix_aug(
                ctypes.byref(self.desc), self._sp_ref(), ctypes.byref(self._aug), L.ptr(self._filt), L.ptr(c.pool),
                L.ptr(c.off), L.ptr(self.plan), L.ptr(self.speed), None if b is None else L.ptr(b.pool),
                None if b is None else L.ptr(b.roff), L.ptr(self.rir), None if n is None else L.ptr(n.pool),
                None if n is None else L.ptr(n.off), L.ptr(self.nplan), L.ptr(self.gains), L.ptr(self.ngain),
                L.ptr(sources), L.ptr(mixture), L.ptr(noise_out), L.ptr(self.status), L.ptr(self._ws),
                self._ws.numel(), L.stream_handle(c.device)), "ctn_dmix_mix_aug")
            return mixture, sources
        if self.ratios is not None:
            L.check(self._lib.ctn_dmix_mix_sp(ctypes.byref(self.desc), ctypes.byref(self._sp), L.ptr(self._filt),
                                              L.ptr(c.pool), L.ptr(c.off), L.ptr(self.plan), L.ptr(self.speed),
                                              L.ptr(self.gains), L.ptr(sources), L.ptr(mixture), L.ptr(self.status),
                                              L.ptr(self._ws), self._ws.numel(), L.stream_handle(c.device)),
                    "ctn_dmix_mix_sp")
            return mixture, sources
        L.check(self._lib.ctn_dmix_mix(ctypes.byref(self.desc), L.ptr(c.pool), L.ptr(c.off), L.ptr(self.plan),
                                       L.ptr(self.gains), L.ptr(sources), L.ptr(mixture), L.ptr(self.status),
                                       L.ptr(self._ws), self._ws.numel(), L.stream_handle(c.device)), "ctn_dmix_mix")
        return mixture, sources

    def batch(self, step):
        """-> (mixture [M, T], lengths [M] int64, sources [M, C, T]) of training step `step`."""
        self.draw(self.first_sample(step))
        mixture, sources = self.mix()
        return mixture, self.lengths, sources


class DynamicMixLoader:
    """Stands where the training AudioDataLoader stands: iterating yields steps_per_epoch
    batches; step = epoch * steps_per_epoch + i, so a resumed run continues the sequence.
    It is its own `sampler` (the solver calls loader.sampler.set_epoch)."""

    def __init__(self, mixer, steps_per_epoch):
        if steps_per_epoch < 1:
            raise ValueError(f"steps_per_epoch={steps_per_epoch}")
        self.mixer, self.steps_per_epoch, self.epoch = mixer, int(steps_per_epoch), 0
        self.sampler = self

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def step_of(self, i):
        return self.epoch * self.steps_per_epoch + i

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        for i in range(self.steps_per_epoch):
            yield self.mixer.batch(self.step_of(i))
