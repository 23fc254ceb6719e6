"""BSS Eval v3 source metrics (SDR / SIR / SAR) without mir_eval.

The reference's evaluate.py computes SDRi with ``mir_eval.separation.
bss_eval_sources`` (evaluate.py:10,90-105), a dependency this image does not
have.  This is a from-scratch restatement of that published
algorithm — E. Vincent, R. Gribonval, C. Fevotte, "Performance measurement in
blind audio source separation", IEEE TASLP 14(4), 2006, as implemented by
mir_eval 0.6/0.7 (``bss_eval_sources`` with ``compute_permutation=True``):

* each estimate is decomposed against the references with time-invariant
  distortion filters of ``flen`` = 512 taps: s_true (the reference, zero-padded
  by flen-1), e_spat (its filtered version minus itself), e_interf (what the
  other references' filters add), e_artif (the rest of the estimate);
* the projections solve the normal equations G c = D, where G holds the inner
  products of all delayed references and D those with the estimate, both taken
  from FFT cross-correlations;
* SDR = 10 log10(|s_true+e_spat|^2 / |e_interf+e_artif|^2),
  SIR = 10 log10(|s_true+e_spat|^2 / |e_interf|^2),
  SAR = 10 log10(|s_true+e_spat+e_interf|^2 / |e_artif|^2);
* the estimate-to-source assignment is the permutation with the largest mean SIR.

Parity with mir_eval is UNPINNED (mir_eval is not installed and no fixture of
its output exists in the reference); tests/test_pipeline.py checks the
metric's defining properties instead (exact estimates, filtered estimates,
additive noise at a known SNR, permutation recovery).

``bss_criteria_device`` / ``bss_eval_sources_batch`` (below) run the same decomposition
for a padded batch on the device (csrc/ctn_bss.hip); the functions above
stay the host restatement they are tested against (tests/test_gpu_bss_eval.py).
"""
from __future__ import annotations

import itertools

import numpy as np
from scipy.linalg import toeplitz
from scipy.signal import fftconvolve

FLEN = 512


def _project(refs: np.ndarray, est: np.ndarray, flen: int) -> np.ndarray:
    """Least-squares projection of est onto all flen-tap filtered versions of refs
    [nsrc, T] -> [T + flen - 1]."""
    nsrc, T = refs.shape
    refs_p = np.hstack((refs, np.zeros((nsrc, flen - 1))))
    est_p = np.hstack((est, np.zeros(flen - 1)))
    n_fft = int(2 ** np.ceil(np.log2(T + flen - 1.0)))
    sf = np.fft.fft(refs_p, n=n_fft, axis=1)
    sef = np.fft.fft(est_p, n=n_fft)
    G = np.zeros((nsrc * flen, nsrc * flen))
    for i in range(nsrc):
        for j in range(i, nsrc):
            ssf = np.real(np.fft.ifft(sf[i] * np.conj(sf[j])))
            ss = toeplitz(np.hstack((ssf[0], ssf[-1:-flen:-1])), r=ssf[:flen])
            G[i * flen:(i + 1) * flen, j * flen:(j + 1) * flen] = ss
            G[j * flen:(j + 1) * flen, i * flen:(i + 1) * flen] = ss.T
    D = np.zeros(nsrc * flen)
    for i in range(nsrc):
        ssef = np.real(np.fft.ifft(sf[i] * np.conj(sef)))
        D[i * flen:(i + 1) * flen] = np.hstack((ssef[0], ssef[-1:-flen:-1]))
    try:
        C = np.linalg.solve(G, D).reshape(flen, nsrc, order="F")
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0].reshape(flen, nsrc, order="F")
    sproj = np.zeros(T + flen - 1)
    for i in range(nsrc):
        sproj += fftconvolve(C[:, i], refs_p[i])[:T + flen - 1]
    return sproj


def _decompose(refs: np.ndarray, est: np.ndarray, j: int, flen: int):
    """(s_true, e_spat, e_interf, e_artif) of estimate `est` against reference j."""
    T = est.size
    s_true = np.hstack((refs[j], np.zeros(flen - 1)))
    e_spat = _project(refs[j:j + 1], est, flen) - s_true
    e_interf = _project(refs, est, flen) - s_true - e_spat
    e_artif = -s_true - e_spat - e_interf
    e_artif[:T] += est
    return s_true, e_spat, e_interf, e_artif


def _db(num: float, den: float) -> float:
    return np.inf if den == 0 else 10.0 * np.log10(num / den)


def _criteria(s_true, e_spat, e_interf, e_artif):
    s_filt = s_true + e_spat
    sdr = _db(np.sum(s_filt ** 2), np.sum((e_interf + e_artif) ** 2))
    sir = _db(np.sum(s_filt ** 2), np.sum(e_interf ** 2))
    sar = _db(np.sum((s_filt + e_interf) ** 2), np.sum(e_artif ** 2))
    return sdr, sir, sar


def bss_eval_sources(reference_sources, estimated_sources, compute_permutation=True, flen=FLEN):
    """reference_sources, estimated_sources [nsrc, T] (or [T]) -> (sdr, sir, sar, perm),
    each [nsrc]; perm[j] = the estimate assigned to reference j (mir_eval's popt)."""
    refs = np.atleast_2d(np.asarray(reference_sources, dtype=np.float64))
    ests = np.atleast_2d(np.asarray(estimated_sources, dtype=np.float64))
    if refs.shape != ests.shape:
        raise ValueError(f"shape mismatch: references {refs.shape}, estimates {ests.shape}")
    if refs.shape[1] < flen:
        raise ValueError(f"signals of {refs.shape[1]} samples are shorter than the {flen}-tap filters")
    if np.any(np.all(refs == 0, axis=1)):
        raise ValueError("a reference source is all zeros (undefined SDR)")
    n = refs.shape[0]
    if not compute_permutation:
        out = np.array([_criteria(*_decompose(refs, ests[j], j, flen)) for j in range(n)])
        return out[:, 0], out[:, 1], out[:, 2], np.arange(n)
    sdr, sir, sar = (np.empty((n, n)) for _ in range(3))
    for je in range(n):
        for jt in range(n):
            sdr[je, jt], sir[je, jt], sar[je, jt] = _criteria(*_decompose(refs, ests[je], jt, flen))
    perms = list(itertools.permutations(range(n)))
    dum = np.arange(n)
    best = perms[int(np.argmax([np.mean(sir[list(p), dum]) for p in perms]))]
    idx = (list(best), dum)
    return sdr[idx], sir[idx], sar[idx], np.asarray(best)


# ----------------------------------------------------------------------------
# Device path (csrc/ctn_bss.hip through ctn_bss_eval): the same decomposition for a ragged
# batch, direct-form fp64 lag correlations and one Cholesky factorisation per
# (utterance, system) instead of FFT correlations and one LU solve per (estimate, reference).
# ----------------------------------------------------------------------------
WS_LIMIT = 1 << 30          # bytes of library workspace per call; larger batches are split


def _lengths_tensor(lengths, M, T, device):
    import torch
    if lengths is None:
        return torch.full((M,), T, dtype=torch.int32, device=device)
    lengths = torch.as_tensor(lengths).to(device=device, dtype=torch.int32).reshape(-1)
    if lengths.numel() != M:
        raise ValueError(f"{lengths.numel()} lengths for {M} utterances")
    return lengths.contiguous()


def bss_criteria_device(refs, sigs, lengths=None, flen=FLEN):
    """refs [M, C, T], sigs [M, E, T] (device tensors; utterance m uses its first lengths[m]
    samples, the rest is never read) -> (sdr, sir, sar), each [M, E, C] fp64 on the device:
    the criteria of signal e against reference j, and status [M] (1: a Gram matrix of the
    utterance was numerically rank-deficient, its row is meaningless)."""
    import ctypes

    import torch

    import ctn_lib as L
    L.require_device(refs, "bss_criteria_device")
    L.require_device(sigs, "bss_criteria_device")
    if refs.dim() != 3 or sigs.dim() != 3 or refs.shape[0] != sigs.shape[0] or refs.shape[2] != sigs.shape[2]:
        raise ValueError(f"shape mismatch: references {tuple(refs.shape)}, signals {tuple(sigs.shape)}")
    refs, sigs = refs.float().contiguous(), sigs.float().contiguous()
    (M, C, T), E = refs.shape, sigs.shape[1]
    lengths = _lengths_tensor(lengths, M, T, refs.device)
    lib = L.load()
    energies = torch.empty(M, E, C, 5, dtype=torch.float64, device=refs.device)
    status = torch.empty(M, dtype=torch.int32, device=refs.device)
    one = lib.ctn_bss_workspace_bytes(ctypes.byref(L.BssDesc(1, C, E, T, flen)))
    if one == 0:                  # unsupported shape: let the entry point name the reason
        L.check(lib.ctn_bss_eval(ctypes.byref(L.BssDesc(1, C, E, T, flen)), None, None, None, None, None, None, 0,
                                 None), "ctn_bss_eval")
    step = max(1, min(M, WS_LIMIT // one, 65535))
    ws = L.workspace(lib.ctn_bss_workspace_bytes(ctypes.byref(L.BssDesc(step, C, E, T, flen))), refs.device)
    for m0 in range(0, M, step):
        m1 = min(M, m0 + step)
        d = L.BssDesc(m1 - m0, C, E, T, flen)
        L.check(lib.ctn_bss_eval(ctypes.byref(d), L.ptr(refs[m0:m1]), L.ptr(sigs[m0:m1]), L.ptr(lengths[m0:m1]),
                                 L.ptr(energies[m0:m1]), L.ptr(status[m0:m1]), L.ptr(ws), ws.numel(),
                                 L.stream_handle(refs.device)), "ctn_bss_eval")
    inf = torch.full_like(energies[..., 0], float("inf"))

    def db(num, den):             # _db: a zero denominator gives +inf
        return torch.where(den == 0, inf, 10.0 * torch.log10(num / den))
    v = energies.unbind(-1)
    return db(v[0], v[2]), db(v[0], v[1]), db(v[3], v[4]), status


def _check_batch(refs, ests, lengths, flen):
    """The ValueErrors of bss_eval_sources for a padded batch -> lengths as a list."""
    import torch
    if refs.dim() != 3 or refs.shape != ests.shape:
        raise ValueError(f"shape mismatch: references {tuple(refs.shape)}, estimates {tuple(ests.shape)}")
    M, C, T = refs.shape
    lengths = _lengths_tensor(lengths, M, T, refs.device)
    n = lengths.tolist()
    if max(n) > T or min(n) < flen:
        bad = min(n) if min(n) < flen else max(n)
        raise ValueError(f"signals of {bad} samples are shorter than the {flen}-tap filters" if bad < flen else
                         f"length {bad} exceeds the {T} samples of the batch")
    inside = torch.arange(T, device=refs.device).unsqueeze(0) < lengths.unsqueeze(1)          # [M, T]
    if not bool(((refs != 0) & inside.unsqueeze(1)).any(-1).all()):
        raise ValueError("a reference source is all zeros (undefined SDR)")
    return lengths, n


def _assign(sdr, sir, sar, compute_permutation):
    """[E >= C, C] criteria of one utterance (row e: estimate e) -> bss_eval_sources' result."""
    n = sdr.shape[1]
    dum = np.arange(n)
    best = tuple(range(n))
    if compute_permutation:
        perms = list(itertools.permutations(range(n)))
        best = perms[int(np.argmax([np.mean(sir[list(p), dum]) for p in perms]))]
    idx = (list(best), dum)
    return sdr[idx], sir[idx], sar[idx], np.asarray(best)


def _on_host(status, n, C, flen):
    """Utterances scored by the host routine: flagged by the library, or with fewer samples
    than unknowns (lengths + flen - 1 < C * flen: the Gram matrix is rank-deficient by
    construction and the host's solve / lstsq decides the result)."""
    return [bool(status[m]) or n[m] + flen - 1 < C * flen for m in range(len(n))]


def bss_eval_sources_batch(reference_sources, estimated_sources, lengths=None, compute_permutation=True, flen=FLEN):
    """bss_eval_sources of every utterance of a padded batch, computed on the device:
    reference_sources, estimated_sources [M, C, T] device tensors, lengths [M] (None: T)
    -> (sdr, sir, sar, perm), numpy arrays [M, C]; row m is bss_eval_sources(refs[m, :,
    :lengths[m]], ests[m, :, :lengths[m]], compute_permutation, flen)."""
    refs, ests = reference_sources, estimated_sources
    lengths, n = _check_batch(refs, ests, lengths, flen)
    M, C, _ = refs.shape
    sdr, sir, sar, status = (t.cpu().numpy() for t in bss_criteria_device(refs, ests, lengths, flen))
    out = [np.empty((M, C)) for _ in range(3)] + [np.empty((M, C), dtype=np.int64)]
    for m, host in enumerate(_on_host(status, n, C, flen)):
        if host:
            res = bss_eval_sources(refs[m, :, :n[m]].double().cpu().numpy(), ests[m, :, :n[m]].double().cpu().numpy(),
                                   compute_permutation, flen)
        else:
            res = _assign(sdr[m], sir[m], sar[m], compute_permutation)
        for o, r in zip(out, res):
            o[m] = r
    return tuple(out)
