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


def plan_host(off, spk, elig, M, C, T, seed=0, first_sample=0, level_db=(-2.5, 2.5), max_tries=16):
    """The plan ctn_dmix_draw writes: a [M, C] array of PLAN_DTYPE."""
    off, spk, elig = np.asarray(off, np.int64), np.asarray(spk, np.int32), np.asarray(elig, np.int32)
    U, E = len(spk), len(elig)
    lo, hi = np.float32(level_db[0]), np.float32(level_db[1])
    key = (int(seed) & _U32, (int(seed) >> 32) & _U32)
    plan = np.zeros((M, C), dtype=PLAN_DTYPE)
    for m in range(M):
        g = (int(first_sample) + m) & 0xFFFFFFFFFFFFFFFF
        taken = []                                       # speakers of the accepted valid slots
        for c in range(C):
            for j in range(max_tries):
                r = philox4x32_10((g & _U32, g >> 32, c, j), key)
                utt = int(elig[(r[0] * E) >> 32])
                level = lo + (hi - lo) * (np.float32(r[2] >> 8) * np.float32(2.0 ** -24))
                e = (-1, 0, level, j + 1)
                n = int(off[utt + 1] - off[utt]) - T + 1 if 0 <= utt < U else 0
                if n < 1 or n > 0x7FFFFFFF:
                    sp = None
                    break
                e = (utt, (r[1] * n) >> 32, level, j + 1)
                sp = int(spk[utt])
                if sp not in taken:
                    break
            plan[m, c] = e
            if sp is not None and e[0] >= 0:
                taken.append(sp)
    return plan


def _segment(pool, off, e, T):
    """fp32 samples of a plan entry, or None for an entry that must not be read."""
    U = len(off) - 1
    utt, start = int(e["utt"]), int(e["start"])
    if not 0 <= utt < U or start < 0 or start + T > int(off[utt + 1] - off[utt]):
        return None
    x = pool[int(off[utt]) + start:int(off[utt]) + start + T]
    if x.dtype == np.int16:
        return x.astype(np.float32) * np.float32(2.0 ** -15)
    return x.astype(np.float32, copy=False)


def mix_host(pool, off, plan, T, level_mode=0, peak=0.9, gains=None):
    """ctn_dmix_mix on the host.  pool: int16 or float32 [n]; plan: [M, C] PLAN_DTYPE.

    -> dict(gains [M, C] float64: the gains in fp64 arithmetic; p [M] float64: the
    unguarded mixture's peak; sources [M, C, T], mixture [M, T] float32; status [M] int32).
    sources and mixture follow the exactness contract with the fp32 gains `gains` when
    given (a device call's read-back gains), else with the fp64 gains rounded to fp32."""
    off = np.asarray(off, np.int64)
    M, C = plan.shape
    g64, p64 = np.zeros((M, C)), np.zeros(M)
    sources, mixture = np.zeros((M, C, T), np.float32), np.zeros((M, T), np.float32)
    status = np.zeros(M, np.int32)
    for m in range(M):
        xs = [_segment(pool, off, plan[m, c], T) for c in range(C)]
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


def plan_to_numpy(plan):
    """Device plan tensor (int32 [M, C, 4]) -> [M, C] array of PLAN_DTYPE."""
    a = plan.detach().cpu().numpy()
    return a.view(PLAN_DTYPE).reshape(a.shape[0], a.shape[1])


def plan_from_numpy(plan, device):
    import torch
    a = np.ascontiguousarray(plan, dtype=PLAN_DTYPE)
    return torch.from_numpy(a.view(np.int32).reshape(a.shape[0], a.shape[1], 4).copy()).to(device)


class DynamicMixer:
    """Draws and mixes batches of M rows, C speakers, T samples on the corpus's device.

    level_mode 0: gain 10^(level_db / 20) on the stored waveform; 1: relative to the
    segment's RMS (floored at 1e-4).  level_db: (lo, hi) of the uniform level draw.
    peak > 0: a row whose mixture would exceed it is scaled down to it."""

    def __init__(self, corpus, M, C, T, seed=0, level_mode=0, level_db=(-2.5, 2.5), peak=0.9, max_tries=16,
                 rank=0, world=1):
        import torch

        import ctn_lib as L
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world size {world}")
        L.require_device(corpus.pool, "DynamicMixer")
        self.corpus, self.M, self.C, self.T = corpus, int(M), int(C), int(T)
        self.rank, self.world = int(rank), int(world)
        self.elig, self.elig_host = corpus.eligible(self.T, self.C)
        self.desc = L.DmixDesc(M=self.M, C=self.C, T=self.T, n_utts=corpus.n_utts, n_elig=len(self.elig_host),
                               pool_dtype=corpus.pool_dtype, level_mode=int(level_mode), max_tries=int(max_tries),
                               level_lo_db=float(level_db[0]), level_hi_db=float(level_db[1]), peak=float(peak),
                               seed=int(seed) & 0xFFFFFFFFFFFFFFFF)
        self._lib = L.load()
        nbytes = self._lib.ctn_dmix_workspace_bytes(ctypes.byref(self.desc))
        if nbytes == 0:
            L.check(self._lib.ctn_dmix_draw(ctypes.byref(self.desc), None, None, None, 0, None, 0, None, None),
                    "DynamicMixer")                     # raises with the library's reason
        dev = corpus.device
        self._ws = L.workspace(nbytes, dev)
        self.plan = torch.zeros(self.M, self.C, 4, dtype=torch.int32, device=dev)
        self.gains = torch.zeros(self.M, self.C, dtype=torch.float32, device=dev)
        self.status = torch.zeros(self.M, dtype=torch.int32, device=dev)
        self.lengths = torch.full((self.M,), self.T, dtype=torch.int64, device=dev)

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
        tensor of one element, to which `advance` is then added on the device)."""
        import torch

        import ctn_lib as L
        c = self.corpus
        if counter is not None:
            self._checked(counter, "counter", torch.int64, (1,))
        L.check(self._lib.ctn_dmix_draw(ctypes.byref(self.desc), L.ptr(c.off), L.ptr(c.spk), L.ptr(self.elig),
                                        int(first_sample), L.ptr(counter), int(advance), L.ptr(self.plan),
                                        L.stream_handle(c.device)), "ctn_dmix_draw")
        return self.plan

    def mix(self, plan=None, sources=None, mixture=None):
        """Mix `plan` (default: the last drawn) -> (mixture [M, T], sources [M, C, T])."""
        import torch

        import ctn_lib as L
        c = self.corpus
        if plan is not None:
            self.plan = self._checked(plan, "plan", torch.int32, (self.M, self.C, 4))
        if sources is None:
            sources = torch.empty(self.M, self.C, self.T, dtype=torch.float32, device=c.device)
        if mixture is None:
            mixture = torch.empty(self.M, self.T, dtype=torch.float32, device=c.device)
        self._checked(sources, "sources", torch.float32, (self.M, self.C, self.T))
        self._checked(mixture, "mixture", torch.float32, (self.M, self.T))
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
