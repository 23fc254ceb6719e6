"""MixIT loss (mixture-invariant training: Wisdom et al., "Unsupervised sound separation
using mixture invariant training", NeurIPS 2020) on MI355X.

Two recordings are added into a mixture of mixtures (MoM); the model separates the MoM into
C outputs; the loss assigns every output to one of the two recordings, takes the best of the
2^C assignments, and scores the two remixed sums against the recordings.  No isolated
sources are needed.  ``cal_mixit_loss`` runs the HIP kernels of ``libctn_hip.so``
(ctn_mixit_forward / ctn_mixit_backward, csrc/ctn_mixit.hip): one fp64 statistics pass over
the audio, a search over all assignments from the statistics alone, one element-wise
backward.  The definition is in DESIGN.md §27 and include/ctn.h.

``mixit_host`` is the fp64 numpy restatement that the tests compare against; it forms every
remixed sum explicitly.  It is test infrastructure, not a fallback.
"""
from __future__ import annotations

import numpy as np
import torch

import ctn_ops as ops

EPS = 1e-8
LOSSES = ("snr", "si_snr")


def cal_mixit_loss(mixtures, estimate_source, lengths, loss="snr", snr_max=30.0):
    """mixtures [M, 2, T] (the two recordings of each MoM), estimate_source [M, C, T]
    (2 <= C <= 8), lengths [M] -> (loss, max_snr [M, 1], assign [M], remix [M, 2, T]).
    Bit c of assign[m] is the recording that output c goes to; remix holds the two remixed
    sums under it (zero beyond each length).  estimate_source is left as it is."""
    return ops.MixITFn.apply(mixtures, estimate_source, lengths, loss, snr_max)


def mom_pairs(mixture, lengths):
    """mixture [2M', T] (or 2M'+1: an odd last utterance is dropped), lengths ->
    (mom [M', T], refs [M', 2, T], lengths [M']): utterances 2m and 2m+1 become the two
    recordings of MoM m, whose length is the longer of the two."""
    n = mixture.size(0) // 2
    refs = mixture[:2 * n].reshape(n, 2, mixture.size(-1))
    lens = lengths[:2 * n].reshape(n, 2).max(dim=1).values
    return refs.sum(dim=1), refs.contiguous(), lens


def _snr_host(x, y, loss, tau):
    """One recording x against one remixed sum y (fp64, already cut to the length)."""
    if loss == "snr":
        X = np.sum(x * x)
        R = np.sum((x - y) ** 2)
        return 10.0 * np.log10((X + EPS) / (R + tau * X + EPS))
    xc, yc = x - np.mean(x), y - np.mean(y)
    D, Et, Ee = np.sum(xc * yc), np.sum(xc * xc), np.sum(yc * yc)
    Pp = D * D * Et / (Et + EPS) ** 2
    Ne = Ee - 2.0 * D * D / (Et + EPS) + D * D * Et / (Et + EPS) ** 2
    return 10.0 * np.log10(Pp / (Ne + EPS) + EPS)


def mixit_host(mixtures, est, lengths, loss="snr", snr_max=30.0):
    """fp64 numpy restatement: every assignment's remixed sums are formed sample by sample
    (no Gram matrix).  -> dict(scores [M, 2^C], assign [M], max_snr [M], loss, remix
    [M, 2, T] (fp32, added in ascending channel order))."""
    if loss not in LOSSES:
        raise ValueError(f"MixIT loss {loss!r}: one of {LOSSES}")
    x32 = np.ascontiguousarray(torch.as_tensor(mixtures).detach().cpu().numpy(), dtype=np.float32)
    e32 = np.ascontiguousarray(torch.as_tensor(est).detach().cpu().numpy(), dtype=np.float32)
    lens = [int(v) for v in torch.as_tensor(lengths).cpu().tolist()]
    M, C, T = e32.shape
    tau = 10.0 ** (-float(snr_max) / 10.0)
    scores = np.zeros((M, 1 << C))
    remix = np.zeros((M, 2, T), dtype=np.float32)
    for m in range(M):
        n = min(lens[m], T)
        x, e = x32[m, :, :n].astype(np.float64), e32[m, :, :n].astype(np.float64)
        for p in range(1 << C):
            y = np.zeros((2, n))
            for c in range(C):
                y[(p >> c) & 1] += e[c]
            with np.errstate(invalid="ignore", divide="ignore"):
                scores[m, p] = 0.5 * (_snr_host(x[0], y[0], loss, tau) + _snr_host(x[1], y[1], loss, tau))
    assign = np.argmax(scores, axis=1)              # the first maximum in ascending p
    for m in range(M):
        n = min(lens[m], T)
        for c in range(C):
            k = (int(assign[m]) >> c) & 1
            remix[m, k, :n] = remix[m, k, :n] + e32[m, c, :n]
    max_snr = scores[np.arange(M), assign]
    return dict(scores=scores, assign=assign.astype(np.int64), max_snr=max_snr, loss=-float(np.mean(max_snr)),
                remix=remix)
