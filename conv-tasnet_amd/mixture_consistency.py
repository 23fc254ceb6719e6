"""Mixture-consistency projection (Wisdom et al., "Differentiable consistency constraints
for improved deep speech enhancement", ICASSP 2019) on MI355X.

A separator's C outputs need not add up to its input.  The projection spreads the residual
``r = x - sum_c s_c`` over the outputs, ``y_c = s_c + w_c r``, so that they do, exactly: with
weights that sum to one, ``sum_c y_c = x``.  ``uniform`` uses ``w_c = 1 / C``; ``power`` uses
``w_c = (p_c + EPS) / (sum_j p_j + C EPS)`` with ``p_c`` the energy of output c over the
utterance, so that loud outputs take most of the residual and silent ones stay silent.
Samples at or past an utterance's length pass through unchanged.  Every MixIT recipe puts
this layer on the model's outputs (``ConvTasNet(..., mixture_consistency='power')``).

``mixture_consistency`` runs the HIP kernels of ``libctn_hip.so`` (ctn_mixcon_forward /
ctn_mixcon_backward, csrc/ctn_mixcon.hip); it is differentiable in the outputs and in the
mixture.  The definition is in DESIGN.md §28 and include/ctn.h.

``mixture_consistency_host`` is the fp64 numpy restatement of the forward and of the
backward formula that the tests compare against.  It is test infrastructure, not a fallback.
"""
from __future__ import annotations

import numpy as np
import torch

import ctn_ops as ops

EPS = 1e-8
MODES = ("uniform", "power")
MIN_C, MAX_C = 2, 16


def check_mode(mode, allow_none=False):
    """A ValueError for anything but the supported modes (and 'none' where a caller allows it)."""
    if mode in MODES or (allow_none and mode == "none"):
        return mode
    raise ValueError(f"mixture consistency {mode!r}: one of {(('none',) if allow_none else ()) + MODES}")


def mixture_consistency(mixture, est, lengths=None, mode="uniform"):
    """mixture [M, T], est [M, C, T] contiguous fp32 (2 <= C <= 16), lengths [M] or None (= T)
    -> [M, C, T]: the outputs projected so that they sum to the mixture at t < length;
    est is left as it is."""
    return ops.MixConFn.apply(mixture, est, lengths, check_mode(mode))[0]


def weights(mixture, est, lengths=None, mode="uniform"):
    """The projection's weights w [M, C] in fp64, as the device worked them out."""
    M, C, _ = est.shape
    if check_mode(mode) == "uniform":
        return torch.full((M, C), 1.0 / C, dtype=torch.float64, device=est.device)
    with torch.no_grad():
        return ops.MixConFn.apply(mixture, est, lengths, mode)[1][:, :C].clone()


def _host_inputs(mixture, est, lengths):
    x = np.ascontiguousarray(torch.as_tensor(mixture).detach().cpu().numpy(), dtype=np.float32).astype(np.float64)
    s = np.ascontiguousarray(torch.as_tensor(est).detach().cpu().numpy(), dtype=np.float32).astype(np.float64)
    M, C, T = s.shape
    if x.shape != (M, T):
        raise ValueError(f"mixture {x.shape} must be [M, T] for estimates {s.shape} [M, C, T]")
    lens = [T] * M if lengths is None else [min(max(int(v), 0), T) for v in torch.as_tensor(lengths).cpu().tolist()]
    return x, s, lens


def mixture_consistency_host(mixture, est, lengths=None, mode="uniform", grad_out=None):
    """fp64 numpy restatement, nothing rounded -> dict(out [M, C, T], w [M, C], D [M]) and, with
    grad_out = dL/d out [M, C, T], also g_est [M, C, T] and g_mixture [M, T] by the backward
    formula of DESIGN.md §28."""
    check_mode(mode)
    x, s, lens = _host_inputs(mixture, est, lengths)
    M, C, T = s.shape
    out = s.copy()
    w = np.full((M, C), 1.0 / C)
    D = np.zeros(M)
    r = np.zeros((M, T))
    for m, n in enumerate(lens):
        if mode == "power":
            p = np.sum(s[m, :, :n] ** 2, axis=1)
            D[m] = np.sum(p) + C * EPS
            w[m] = (p + EPS) / D[m]
        acc = np.zeros(n)
        for c in range(C):                                   # ascending j
            acc = acc + s[m, c, :n]
        r[m, :n] = x[m, :n] - acc
        out[m, :, :n] = s[m, :, :n] + w[m][:, None] * r[m, :n]
    res = dict(out=out, w=w, D=D)
    if grad_out is not None:
        g = np.ascontiguousarray(torch.as_tensor(grad_out).detach().cpu().numpy()).astype(np.float64)
        gs, gx = g.copy(), np.zeros((M, T))
        for m, n in enumerate(lens):
            G = np.zeros(n)
            for c in range(C):
                G = G + w[m, c] * g[m, c, :n]
            gs[m, :, :n] = g[m, :, :n] - G
            if mode == "power":
                a = np.sum(g[m, :, :n] * r[m, :n], axis=1)
                k = 2.0 * (a - np.sum(w[m] * a)) / D[m]
                gs[m, :, :n] += s[m, :, :n] * k[:, None]
            gx[m, :n] = G
        res.update(g_est=gs, g_mixture=gx)
    return res
