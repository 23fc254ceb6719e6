"""PIT with silent sources (Wisdom et al., "What's all the FUSS about free universal sound
separation data?", ICASSP 2021, §4) on MI355X: one model with C outputs is trained on, and
scored against, recordings with 1 ... C (or no) speaking sources.

A reference that is exactly zero inside the utterance's length is *silent*.  An output paired
with an active reference is scored by SNR (or SI-SNR); an output paired with a silent reference
is scored by how far it lies below the mixture; the permutation is searched over both kinds
together.  ``cal_loss_var`` runs the HIP kernels of ``libctn_hip.so`` (ctn_pitvar_forward /
ctn_pitvar_backward, csrc/ctn_pitvar.hip): one fp64 statistics pass over the audio, the C x C
scores and all C! permutations from the statistics alone, one element-wise backward.  The
definition is in DESIGN.md §29 and include/ctn.h.

``pit_var_host`` is the fp64 numpy restatement that the tests compare against; it forms every
residual sample by sample.  It is test infrastructure, not a fallback.
"""
from __future__ import annotations

from itertools import permutations

import numpy as np
import torch

import ctn_ops as ops
from mixit_criterion import _snr_host

EPS = 1e-8
LOSSES = ("snr", "si_snr")


def cal_loss_var(source, estimate_source, source_lengths, mixture=None, loss="snr", snr_max=30.0,
                 inactive_snr_max=20.0):
    """source, estimate_source [M, C, T] (2 <= C <= 8), source_lengths [M], mixture [M, T] or None
    (then the sum of the sources) -> (loss, max_snr [M, 1], perm [M, C] int64, active [M, C] bool).
    perm[m, i] is the reference of output i; active[m, j] says whether reference j has a non-zero
    sample inside the length.  Differentiable in estimate_source through loss and max_snr;
    estimate_source is left as it is."""
    return ops.PITVarFn.apply(source, estimate_source, source_lengths, mixture, loss, snr_max, inactive_snr_max)


def _inactive_host(x, e, tau0):
    """An output e paired with a silent reference, against the mixture x (fp64, cut to the length)."""
    X = np.sum(x * x)
    return 10.0 * np.log10((X + EPS) / (np.sum(e * e) + tau0 * X + EPS))


def pit_var_host(source, est, lengths, mixture=None, loss="snr", snr_max=30.0, inactive_snr_max=20.0):
    """fp64 numpy restatement: every residual is formed sample by sample (no Gram matrix) and
    itertools.permutations is enumerated, the first maximum kept.  -> dict(scores [M, C, C]
    (output i against reference j), perm [M, C], active [M, C] bool, max_snr [M], loss)."""
    if loss not in LOSSES:
        raise ValueError(f"PIT-var loss {loss!r}: one of {LOSSES}")
    s32 = np.ascontiguousarray(torch.as_tensor(source).detach().cpu().numpy(), dtype=np.float32)
    e32 = np.ascontiguousarray(torch.as_tensor(est).detach().cpu().numpy(), dtype=np.float32)
    x32 = None if mixture is None else np.ascontiguousarray(torch.as_tensor(mixture).detach().cpu().numpy(),
                                                            dtype=np.float32)
    lens = [int(v) for v in torch.as_tensor(lengths).cpu().tolist()]
    M, C, T = e32.shape
    tau, tau0 = 10.0 ** (-float(snr_max) / 10.0), 10.0 ** (-float(inactive_snr_max) / 10.0)
    scores = np.zeros((M, C, C))
    active = np.zeros((M, C), dtype=bool)
    perm = np.zeros((M, C), dtype=np.int64)
    max_snr = np.zeros(M)
    for m in range(M):
        n = min(lens[m], T)
        s, e = s32[m, :, :n].astype(np.float64), e32[m, :, :n].astype(np.float64)
        if x32 is None:
            x = np.zeros(n)
            for j in range(C):
                x = x + s[j]
        else:
            x = x32[m, :n].astype(np.float64)
        for j in range(C):
            active[m, j] = np.sum(s[j] * s[j]) > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in range(C):
                for j in range(C):
                    scores[m, i, j] = _snr_host(s[j], e[i], loss, tau) if active[m, j] else \
                        _inactive_host(x, e[i], tau0)
        best, bp = None, None
        for p in permutations(range(C)):
            sv = 0.0
            for i in range(C):
                sv += scores[m, i, p[i]]
            if best is None or sv > best:            # the first maximum
                best, bp = sv, p
        perm[m] = bp
        max_snr[m] = best / C
    return dict(scores=scores, perm=perm, active=active, max_snr=max_snr, loss=-float(np.mean(max_snr)))
