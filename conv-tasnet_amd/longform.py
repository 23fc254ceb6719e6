"""Windowed separation of a recording of any length.

The recording is cut into J overlapping windows of the training length, the windows are
separated as batches by the existing HIP forward, and the per-window outputs P [J, C, W] are
joined on the device (csrc/ctn_stitch.hip): a C x C correlation per boundary in fp64, the
permutation that links each window to the one before it, the chain of those permutations,
and a permuted cross-fade overlap-add.  Memory no longer grows with the recording and a gLN
model is normalised over the segment length it was trained on.

``ChunkedSeparator`` drives model + stitch; ``stitch`` joins window outputs that already
exist.  The ``*_host`` functions restate every step in numpy, in the kernels' summation
order, and are what the device is tested against bit for bit; they are test infrastructure,
not a fallback.

The operation (include/ctn.h has the same text for the C ABI):

* windows: J = 1 if T <= W else 1 + ceil((T - W) / Hs), Hs = W - O; window j is
  x[j Hs : j Hs + W] with zeros past T; every overlap [j Hs, j Hs + O) lies below T;
* S_j[a][b] = sum_{u<O} P[j-1][a][Hs+u] P[j][b][u] in fp64, j = 1 ... J-1 (order: corr_host);
* pi_j maximises sum_a S_j[a][pi_j(a)] over itertools.permutations(range(C)) order, a later
  permutation winning only on ``>``; a non-finite S_j gives the identity and status 1;
* sigma_0 = id, sigma_j(a) = pi_j(sigma_{j-1}(a)); output channel a takes P[j][sigma_j(a)];
* overlaps are cross-faded in fp32, out = fl(fl(fl(1 - f) p) + fl(f c)), the rest is copied.
"""
from __future__ import annotations

import collections
import ctypes
import itertools
import math

import numpy as np
import torch

import ctn_lib as L

MIN_C, MAX_C = 2, 8
CHUNK, THREADS = 2048, 256     # csrc/ctn_stitch.h STITCH_CHUNK, STITCH_THREADS
FADES = ("linear", "hann")

StitchResult = collections.namedtuple("StitchResult", "out perm sigma status sim")


# ----------------------------------------------------------------------------
# shapes and constraints
# ----------------------------------------------------------------------------
def check_shape(W: int, O: int, C: int | None = None, L_: int | None = None):
    """The constraints of the operation; a violation is a ValueError."""
    W, O = int(W), int(O)
    if W < 2 or O < 1 or O > W // 2:
        raise ValueError(f"window {W}, overlap {O}: need 1 <= overlap <= window // 2 (only neighbours overlap)")
    if C is not None and not MIN_C <= int(C) <= MAX_C:
        raise ValueError(f"{C} speakers: the permutation search covers {MIN_C} ... {MAX_C}")
    if L_ is not None:
        if W < L_ or (W - L_) % (L_ // 2) != 0:
            raise ValueError(f"window {W} does not fill whole frames of the model: need window >= L = {L_} and "
                             f"(window - L) % (L // 2) == 0")


def window_count(T: int, W: int, O: int) -> int:
    check_shape(W, O)
    if T < 1:
        raise ValueError(f"recording of {T} samples")
    Hs = W - O
    return 1 if T <= W else 1 + -(-(T - W) // Hs)


def nearest_valid(window_s: float, overlap_s: float, sample_rate: int, L_: int):
    """Seconds -> the nearest (W, O) with W >= L, (W - L) % (L // 2) == 0 and 1 <= O <= W // 2."""
    half = max(L_ // 2, 1)
    W = L_ + max(0, int(round((window_s * sample_rate - L_) / half))) * half
    W = max(W, 2)
    O = min(max(int(round(overlap_s * sample_rate)), 1), W // 2)
    check_shape(W, O, L_=L_)
    return W, O


def fade_table(O: int, fade: str = "linear") -> np.ndarray:
    """fade[O] fp32: computed in fp64, then rounded."""
    u = (np.arange(O, dtype=np.float64) + 0.5) / O
    if fade == "linear":
        return u.astype(np.float32)
    if fade == "hann":
        return (np.sin(np.pi * u / 2.0) ** 2).astype(np.float32)
    raise ValueError(f"fade {fade!r}: one of {FADES}")


# ----------------------------------------------------------------------------
# host restatement (numpy)
# ----------------------------------------------------------------------------
def frame_host(x, W: int, O: int) -> np.ndarray:
    """x [T] -> windows [J, W] fp32, zeros past T."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    T, Hs = x.shape[0], W - O
    J = window_count(T, W, O)
    pad = np.zeros((J - 1) * Hs + W, dtype=np.float32)
    pad[:T] = x
    return np.stack([pad[j * Hs:j * Hs + W] for j in range(J)])


def _chunk_sums(prod: np.ndarray) -> np.ndarray:
    """prod [..., n * CHUNK] fp64 products -> [..., n] chunk sums in the kernel's order: thread
    t adds u = 1024 h + 4 t + e (h = 0, 1; e = 0 ... 3) in turn from +0, the thread sums go through
    v[l] += v[l + s], s = 32 ... 1 inside each wave and ((w0 + w1) + w2) + w3 across waves."""
    lead = prod.shape[:-1]
    n = prod.shape[-1] // CHUNK
    v = prod.reshape(lead + (n, 2, THREADS, 4))
    acc = np.zeros(lead + (n, THREADS), dtype=np.float64)
    for h in range(2):
        for e in range(4):
            acc = acc + v[..., h, :, e]
    v = acc.reshape(lead + (n, THREADS // 64, 64))
    s = 32
    while s:
        v = v[..., :s] + v[..., s:2 * s]
        s //= 2
    w = v[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def corr_host(P, O: int) -> np.ndarray:
    """P [J, C, W] -> S [J, C, C] fp64 (row 0 zeros) in the correlation kernel's order."""
    P = np.asarray(P, dtype=np.float32)
    J, C, W = P.shape
    check_shape(W, O, C)
    Hs = W - O
    n = -(-O // CHUNK)
    S = np.zeros((J, C, C), dtype=np.float64)
    step = max(1, (1 << 22) // (C * C * n * CHUNK))
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(1, J, step):
            j1 = min(J, j0 + step)
            p = np.zeros((j1 - j0, C, n * CHUNK), dtype=np.float64)
            q = np.zeros_like(p)
            p[..., :O] = P[j0 - 1:j1 - 1, :, Hs:Hs + O]
            q[..., :O] = P[j0:j1, :, :O]
            prod = p[:, :, None, :] * q[:, None, :, :]   # samples at or past O: +0
            part = _chunk_sums(prod)                     # [jb, C, C, n]
            acc = np.zeros(part.shape[:-1], dtype=np.float64)
            for ch in range(n):
                acc = acc + part[..., ch]
            S[j0:j1] = acc
    return S


_PERM_TABLES = {}


def _perm_table(C: int) -> np.ndarray:
    if C not in _PERM_TABLES:
        _PERM_TABLES[C] = np.array(list(itertools.permutations(range(C))), dtype=np.int64)
    return _PERM_TABLES[C]


def perms_host(S):
    """S [J, C, C] -> (perm [J, C] int32, status [J] int32); row 0 is the identity."""
    S = np.asarray(S, dtype=np.float64)
    J, C, _ = S.shape
    tbl = _perm_table(C)
    perm = np.tile(np.arange(C, dtype=np.int32), (J, 1))
    status = np.zeros(J, dtype=np.int32)
    for j in range(1, J):
        if not np.isfinite(S[j]).all():
            status[j] = 1
            continue
        score = S[j, 0, tbl[:, 0]]
        for a in range(1, C):
            score = score + S[j, a, tbl[:, a]]
        perm[j] = tbl[int(np.argmax(score))]          # the first maximiser
    return perm, status


def chain_host(perm) -> np.ndarray:
    """sigma_0 = id, sigma_j(a) = pi_j(sigma_{j-1}(a))."""
    perm = np.asarray(perm)
    sigma = np.empty_like(perm, dtype=np.int32)
    cur = np.arange(perm.shape[1])
    for j in range(perm.shape[0]):
        cur = cur if j == 0 else perm[j][cur]
        sigma[j] = cur
    return sigma


def ola_host(P, sigma, T: int, O: int, fade="linear") -> np.ndarray:
    """Permuted cross-fade overlap-add -> [C, T] fp32 (separately rounded fp32 operations)."""
    P = np.asarray(P, dtype=np.float32)
    J, C, W = P.shape
    Hs = W - O
    f = fade_table(O, fade) if isinstance(fade, str) else np.asarray(fade, dtype=np.float32)
    one = np.float32(1.0)
    out = np.zeros((C, (J - 1) * Hs + W), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(J):
            cur = P[j, np.asarray(sigma[j])]
            lo = j * Hs
            if j == 0:
                out[:, :W] = cur
                continue
            prev = out[:, lo:lo + O]                  # window j-1 at Hs + u, not yet faded
            out[:, lo:lo + O] = ((one - f) * prev).astype(np.float32) + (f * cur[:, :O]).astype(np.float32)
            out[:, lo + O:lo + W] = cur[:, O:]
    return np.ascontiguousarray(out[:, :T])


def stitch_host(P, T: int, O: int, fade="linear") -> StitchResult:
    P = np.asarray(P, dtype=np.float32)
    J, C, W = P.shape
    if J != window_count(T, W, O):
        raise ValueError(f"{J} windows for T={T}, W={W}, O={O}: expected {window_count(T, W, O)}")
    sim = corr_host(P, O)
    perm, status = perms_host(sim)
    sigma = chain_host(perm)
    return StitchResult(ola_host(P, sigma, T, O, fade), perm, sigma, status, sim)


# ----------------------------------------------------------------------------
# device path (libctn_hip.so)
# ----------------------------------------------------------------------------
def _desc(J, C, W, O, T):
    return L.StitchDesc(J=J, C=C, W=W, O=O, T=T)


def _fade_device(O, fade, device):
    f = fade_table(O, fade) if isinstance(fade, str) else np.asarray(fade, dtype=np.float32)
    if f.shape != (O,):
        raise ValueError(f"fade table of shape {f.shape}, overlap {O}")
    return torch.from_numpy(np.ascontiguousarray(f)).to(device)


def frame(x: torch.Tensor, W: int, O: int) -> torch.Tensor:
    """x [T] fp32 on the device -> windows [J, W] (ctn_stitch_frame)."""
    L.require_device(x, "longform.frame")
    x = x.reshape(-1).contiguous().float()
    T = x.numel()
    J = window_count(T, W, O)
    d = _desc(J, MIN_C, W, O, T)
    win = torch.empty((J, W), dtype=torch.float32, device=x.device)
    L.check(L.load().ctn_stitch_frame(ctypes.byref(d), L.ptr(x), L.ptr(win), L.stream_handle(x.device)),
            "ctn_stitch_frame")
    return win


def stitch(P: torch.Tensor, T: int, overlap: int, fade="linear") -> StitchResult:
    """Join window outputs P [J, C, W] (fp32, device) into [C, T]: ctn_stitch_plan + ctn_stitch_ola."""
    L.require_device(P, "longform.stitch")
    if P.dim() != 3:
        raise ValueError(f"P of shape {tuple(P.shape)}: expected [J, C, W]")
    P = P.contiguous().float()
    J, C, W = P.shape
    O, T = int(overlap), int(T)
    check_shape(W, O, C)
    if J != window_count(T, W, O):
        raise ValueError(f"{J} windows for T={T}, W={W}, O={O}: expected {window_count(T, W, O)}")
    dev = P.device
    lib, d, st = L.load(), _desc(J, C, W, O, T), L.stream_handle(dev)
    nbytes = lib.ctn_stitch_workspace_bytes(ctypes.byref(d))
    if nbytes == 0:
        raise L.CtnLibraryError("ctn_stitch_workspace_bytes: " + lib.ctn_last_error().decode(errors="replace"))
    ws = L.workspace(nbytes, dev)
    sim = torch.empty((J, C, C), dtype=torch.float64, device=dev)
    perm = torch.empty((J, C), dtype=torch.int32, device=dev)
    sigma = torch.empty((J, C), dtype=torch.int32, device=dev)
    status = torch.empty((J,), dtype=torch.int32, device=dev)
    out = torch.empty((C, T), dtype=torch.float32, device=dev)
    f = _fade_device(O, fade, dev)
    L.check(lib.ctn_stitch_plan(ctypes.byref(d), L.ptr(P), L.ptr(sim), L.ptr(perm), L.ptr(sigma), L.ptr(status),
                                L.ptr(ws), nbytes, st), "ctn_stitch_plan")
    L.check(lib.ctn_stitch_ola(ctypes.byref(d), L.ptr(P), L.ptr(sigma), L.ptr(f), L.ptr(out), st), "ctn_stitch_ola")
    return StitchResult(out, perm, sigma, status, sim)


class ChunkedSeparator:
    """Separates a recording of any length window by window and stitches on the device.

    ``model`` is any callable [B, W] -> [B, C, W] on the device; for a ``ConvTasNet`` the
    window is checked against its L (whole frames: its F.pad adds nothing) and C.  After
    ``separate`` the attributes ``perm`` (pi), ``sigma``, ``status`` and ``sim`` hold the
    last call's device tensors ([J, C], [J, C], [J], [J, C, C]; row 0 is the first window).
    """

    def __init__(self, model, window: int, overlap: int, batch: int = 8, fade: str = "linear"):
        self.model = model
        self.window, self.overlap, self.batch = int(window), int(overlap), int(batch)
        if self.batch < 1:
            raise ValueError(f"batch {batch}: at least one window per forward")
        if fade not in FADES:
            raise ValueError(f"fade {fade!r}: one of {FADES}")
        self.fade = fade
        check_shape(self.window, self.overlap, getattr(model, "C", None), getattr(model, "L", None))
        self.perm = self.sigma = self.status = self.sim = None

    def windows(self, mixture: torch.Tensor) -> torch.Tensor:
        return frame(mixture, self.window, self.overlap)

    def forward_windows(self, win: torch.Tensor, T: int | None = None) -> torch.Tensor:
        """[J, W] -> P [J, C, W] fp32, one forward per ``batch`` windows.  A ConvTasNet with
        mixture consistency on also gets each window's valid length (T: the recording's
        samples; only the zero-padded last window is shorter than W), so that the padding is
        not projected; any other callable is called as before."""
        if T is not None and getattr(self.model, "mixture_consistency", "none") != "none":
            Hs = self.window - self.overlap
            valid = (T - Hs * torch.arange(win.shape[0], device=win.device)).clamp(0, self.window)
            parts = [self.model(win[b:b + self.batch], valid[b:b + self.batch])
                     for b in range(0, win.shape[0], self.batch)]
        else:
            parts = [self.model(win[b:b + self.batch]) for b in range(0, win.shape[0], self.batch)]
        for p in parts:
            if p.dim() != 3 or p.shape[-1] != self.window:
                raise ValueError(f"model output of shape {tuple(p.shape)}: expected [B, C, {self.window}]")
        return torch.cat(parts, dim=0).float()

    @torch.no_grad()
    def separate(self, mixture: torch.Tensor) -> torch.Tensor:
        """mixture [T] or [1, T] on the device -> estimates [C, T]."""
        L.require_device(mixture, "ChunkedSeparator")
        if mixture.dim() == 2 and mixture.shape[0] == 1:
            mixture = mixture[0]
        if mixture.dim() != 1 or mixture.numel() < 1:
            raise ValueError(f"mixture of shape {tuple(mixture.shape)}: expected [T] or [1, T]")
        T = mixture.numel()
        P = self.forward_windows(self.windows(mixture), T)
        res = stitch(P, T, self.overlap, self.fade)
        self.perm, self.sigma, self.status, self.sim = res.perm, res.sigma, res.status, res.sim
        return res.out

    def flagged(self):
        """Boundaries of the last call whose similarity was not finite (status 1)."""
        return [] if self.status is None else torch.nonzero(self.status).flatten().tolist()


def from_seconds(model, chunk_s: float, overlap_s: float, sample_rate: int, batch: int = 8, fade: str = "linear"):
    """A ChunkedSeparator for a ConvTasNet with seconds rounded to the nearest valid (W, O)."""
    W, O = nearest_valid(chunk_s, overlap_s, sample_rate, model.L)
    return ChunkedSeparator(model, W, O, batch=batch, fade=fade)
