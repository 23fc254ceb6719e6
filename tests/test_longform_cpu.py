"""Windowed separation without a GPU (longform.py): the window arithmetic,
the numpy restatement of the stitch (tie rule, non-finite rule, chain direction, recovery
of planted sources), the constraint checks, and the C entries' argument validation, which
happens before the device is touched."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import longform as lf


# ----------------------------------------------------------------------------
# windows
# ----------------------------------------------------------------------------
W0, O0 = 20, 6
HS0 = W0 - O0
_TS = [1, W0 - 1, W0, W0 + 1] + [W0 + k * HS0 + e for k in (1, 2, 5) for e in (-1, 0, 1)]


@pytest.mark.parametrize("T", _TS)
def test_window_count_and_frames(T):
    J = lf.window_count(T, W0, O0)
    assert J == (1 if T <= W0 else 1 + -(-(T - W0) // HS0))
    assert (J - 1) * HS0 + W0 >= T                       # the windows cover the recording
    if J > 1:
        assert (J - 2) * HS0 + W0 < T                    # and none is superfluous
    for j in range(1, J):
        assert j * HS0 + O0 <= T, "an overlap reaches the padding"
    x = np.arange(1, T + 1, dtype=np.float32)
    win = lf.frame_host(x, W0, O0)
    assert win.shape == (J, W0) and win.dtype == np.float32
    for j in range(J):
        for w in range(W0):
            g = j * HS0 + w
            assert win[j, w] == (x[g] if g < T else 0.0)


def test_window_count_exact_values():
    assert [lf.window_count(T, 20, 6) for T in (1, 19, 20, 21, 34, 35, 48, 49)] == [1, 1, 1, 2, 2, 3, 3, 4]
    assert lf.window_count(4_800_000, 32000, 16000) == 299


# ----------------------------------------------------------------------------
# permutation search
# ----------------------------------------------------------------------------
def _S(J, C, rows):
    S = np.zeros((J, C, C))
    for j, m in rows.items():
        S[j] = np.asarray(m, dtype=np.float64)
    return S


def test_perms_ties_give_first_permutation():
    # every permutation scores the same: the identity, the first in itertools order
    perm, status = lf.perms_host(_S(2, 3, {1: np.ones((3, 3))}))
    assert perm[1].tolist() == [0, 1, 2] and status.tolist() == [0, 0]
    # two maximisers, (1, 0, 2) and (1, 2, 0): the earlier one
    S = np.zeros((3, 3))
    S[0, 1] = 5.0
    perm, _ = lf.perms_host(_S(2, 3, {1: S}))
    order = list(itertools.permutations(range(3)))
    best = [p for p in order if p[0] == 1]
    assert tuple(perm[1]) == best[0] == (1, 0, 2)
    # a unique maximiser that is late in the order
    S = np.zeros((3, 3))
    S[0, 2] = S[1, 1] = S[2, 0] = 1.0
    assert lf.perms_host(_S(2, 3, {1: S}))[0][1].tolist() == [2, 1, 0]


def test_perms_nonfinite_and_silence():
    good = [[0.0, 2.0], [3.0, 0.0]]
    for bad in (np.nan, np.inf, -np.inf):
        S = _S(4, 2, {1: good, 2: [[0.0, bad], [1.0, 0.0]], 3: good})
        perm, status = lf.perms_host(S)
        assert status.tolist() == [0, 0, 1, 0]
        assert perm.tolist() == [[0, 1], [1, 0], [0, 1], [1, 0]]
    perm, status = lf.perms_host(np.zeros((3, 4, 4)))          # all-zero overlaps
    assert (perm == np.arange(4)).all() and not status.any()
    assert perm.dtype == np.int32 and status.dtype == np.int32


def test_corr_host_matches_fsum_and_zero_windows():
    rng = np.random.default_rng(0)
    P = rng.standard_normal((3, 2, 4100)).astype(np.float32)
    O = 2049
    S = lf.corr_host(P, O)
    assert S.shape == (3, 2, 2) and not S[0].any()
    import math
    for j in (1, 2):
        for a in range(2):
            for b in range(2):
                p = P[j - 1, a, 4100 - O:].astype(np.float64)
                q = P[j, b, :O].astype(np.float64)
                assert abs(S[j, a, b] - math.fsum(p * q)) <= 1e-12 * np.abs(p * q).sum()
    perm, status = lf.perms_host(lf.corr_host(np.zeros((4, 3, 64), np.float32), 16))
    assert (perm == np.arange(3)).all() and not status.any()


# ----------------------------------------------------------------------------
# chain
# ----------------------------------------------------------------------------
def test_chain_direction():
    """sigma_j = pi_j o sigma_{j-1} with 3-cycles (which do not commute with the other
    3-cycle's powers in general positions and are not their own inverses)."""
    c1, c2 = [1, 2, 0], [2, 0, 1]
    swap = [1, 0, 2]
    perm = np.array([[0, 1, 2], c1, swap, c1, c2, swap, c1], dtype=np.int32)
    sigma = lf.chain_host(perm)
    want = [list(range(3))]
    rev = [list(range(3))]
    inv = [list(range(3))]
    for j in range(1, len(perm)):
        pi = perm[j].tolist()
        want.append([pi[want[-1][a]] for a in range(3)])            # pi_j(sigma_{j-1}(a))
        rev.append([rev[-1][pi[a]] for a in range(3)])              # sigma_{j-1}(pi_j(a))
        ipi = [pi.index(a) for a in range(3)]
        inv.append([ipi[inv[-1][a]] for a in range(3)])
    assert sigma.tolist() == want
    assert sigma.tolist() != rev and sigma.tolist() != inv
    # every pi_j the same 3-cycle: sigma_j is its j-th power
    sigma = lf.chain_host(np.array([[0, 1, 2]] + [c1] * 4, dtype=np.int32))
    assert sigma.tolist() == [[0, 1, 2], c1, c2, [0, 1, 2], c1]
    assert sigma.tolist() != [[0, 1, 2], c2, c1, [0, 1, 2], c2]     # the inverse chain


# ----------------------------------------------------------------------------
# planted sources
# ----------------------------------------------------------------------------
def plant(src, W, O, rng):
    """Windows of known sources [C, T] with a random channel order per window:
    -> (P [J, C, W], tau [J, C]) with P[j][tau_j[c]] = source c."""
    C, T = src.shape
    Hs = W - O
    J = lf.window_count(T, W, O)
    pad = np.zeros((C, (J - 1) * Hs + W), dtype=np.float32)
    pad[:, :T] = src
    P = np.empty((J, C, W), dtype=np.float32)
    tau = np.empty((J, C), dtype=np.int64)
    for j in range(J):
        tau[j] = rng.permutation(C)
        P[j, tau[j]] = pad[:, j * Hs:j * Hs + W]
    return P, tau


@pytest.mark.parametrize("C,W,O,T,fade", [(2, 64, 32, 64 + 5 * 32, "linear"), (3, 100, 37, 611, "hann"),
                                          (4, 80, 1, 80 + 3 * 79 + 1, "linear"), (3, 50, 25, 31, "linear")])
def test_stitch_host_recovers_planted_sources(C, W, O, T, fade):
    rng = np.random.default_rng(C * 1000 + T)
    src = rng.standard_normal((C, T)).astype(np.float32)
    P, tau = plant(src, W, O, rng)
    res = lf.stitch_host(P, T, O, fade)
    # output channel a is the source that window 0 holds in channel a, all the way through
    want_sigma = np.stack([tau[j][np.argsort(tau[0])] for j in range(P.shape[0])])
    assert (res.sigma == want_sigma).all()
    assert (res.perm[0] == np.arange(C)).all() and not res.status.any()
    want = src[np.argsort(tau[0])]
    assert res.out.shape == (C, T) and res.out.dtype == np.float32
    assert np.abs(res.out - want).max() <= 1e-6 * np.abs(want).max()


def test_fade_tables():
    for O in (1, 7, 64):
        lin, han = lf.fade_table(O, "linear"), lf.fade_table(O, "hann")
        u = (np.arange(O) + 0.5) / O
        assert lin.dtype == np.float32 and (lin == u.astype(np.float32)).all()
        assert (han == (np.sin(np.pi * u / 2) ** 2).astype(np.float32)).all()
        assert np.allclose(han + han[::-1], 1.0, atol=1e-6) and np.allclose(lin + lin[::-1], 1.0, atol=1e-6)


# ----------------------------------------------------------------------------
# constraints
# ----------------------------------------------------------------------------
class _Shape:
    """Stands in for a ConvTasNet's attributes."""

    def __init__(self, L, C):
        self.L, self.C = L, C

    def __call__(self, x):
        raise AssertionError("not called")


def test_constraint_violations_raise():
    for W, O in ((64, 0), (64, 33), (64, -1), (1, 1), (0, 0)):
        with pytest.raises(ValueError):
            lf.check_shape(W, O)
        with pytest.raises(ValueError):
            lf.window_count(100, W, O)
    for C in (1, 9, 0):
        with pytest.raises(ValueError):
            lf.check_shape(64, 32, C)
    with pytest.raises(ValueError):
        lf.window_count(0, 64, 32)
    with pytest.raises(ValueError):
        lf.fade_table(8, "cosine")
    # against a model: W >= L and (W - L) % (L // 2) == 0, 2 <= C <= 8
    lf.ChunkedSeparator(_Shape(20, 2), 32000, 16000)
    lf.ChunkedSeparator(_Shape(4, 3), 200, 100)
    for L_, C, W, O in ((20, 2, 32005, 16000), (20, 2, 10, 5), (20, 1, 32000, 16000), (20, 9, 32000, 16000),
                        (20, 2, 32000, 16001), (20, 2, 32000, 0)):
        with pytest.raises(ValueError):
            lf.ChunkedSeparator(_Shape(L_, C), W, O)
    with pytest.raises(ValueError):
        lf.ChunkedSeparator(_Shape(20, 2), 32000, 16000, batch=0)
    with pytest.raises(ValueError):
        lf.ChunkedSeparator(_Shape(20, 2), 32000, 16000, fade="cosine")
    with pytest.raises(ValueError):
        lf.stitch_host(np.zeros((2, 2, 64), np.float32), 64 + 2 * 32, 32)     # J does not match T
    with pytest.raises(ValueError):
        lf.corr_host(np.zeros((2, 9, 64), np.float32), 32)


def test_nearest_valid_rounding():
    assert lf.nearest_valid(4.0, 2.0, 8000, 20) == (32000, 16000)
    assert lf.nearest_valid(2.0, 1.0, 8000, 20) == (16000, 8000)
    W, O = lf.nearest_valid(1.00037, 0.9, 8000, 20)
    assert (W - 20) % 10 == 0 and abs(W - 8003) <= 5 and O == W // 2
    assert lf.nearest_valid(0.0, 0.0, 8000, 20) == (20, 1)


def test_cpu_tensors_are_refused():
    import torch
    import ctn_lib as L
    with pytest.raises(L.CtnLibraryError):
        lf.stitch(torch.zeros(1, 2, 64), 64, 32)
    with pytest.raises(L.CtnLibraryError):
        lf.ChunkedSeparator(lambda x: x, 64, 32).separate(torch.zeros(100))


# ----------------------------------------------------------------------------
# C ABI: argument checks happen before the device is touched
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


ARG = 1     # include/ctn.h CTN_ERR_ARG


def _d(**kw):
    import ctn_lib as L
    v = dict(J=4, C=2, W=64, O=32, T=64 + 3 * 32)
    v.update(kw)
    return L.StitchDesc(**v)


def test_capi_symbols_exported(lib):
    import ctn_lib as L
    for name in ("ctn_stitch_workspace_bytes", "ctn_stitch_frame", "ctn_stitch_plan", "ctn_stitch_ola"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(L.StitchDesc) == 20


def test_capi_rejects_bad_descriptors(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    ok = _d()
    assert lib.ctn_stitch_workspace_bytes(ctypes.byref(ok)) == 3 * 1 * 4 * 8
    assert lib.ctn_stitch_workspace_bytes(ctypes.byref(_d(J=1, T=64))) > 0
    assert lib.ctn_stitch_workspace_bytes(ctypes.byref(_d(J=2, W=32000, O=16000, T=48000))) == 8 * 4 * 8
    assert lib.ctn_stitch_workspace_bytes(None) == 0
    bad = [_d(C=1), _d(C=9), _d(O=0), _d(O=33), _d(W=1, O=1), _d(T=0), _d(J=3), _d(J=5), _d(J=0), _d(T=-5),
           _d(W=-64), _d(J=1)]
    for d in bad:
        r = ctypes.byref(d)
        assert lib.ctn_stitch_workspace_bytes(r) == 0
        assert lib.ctn_stitch_frame(r, p, p, None) == ARG
        assert lib.ctn_last_error()
        assert lib.ctn_stitch_plan(r, p, p, p, p, p, p, 1 << 16, None) == ARG
        assert lib.ctn_stitch_ola(r, p, p, p, p, None) == ARG
    assert lib.ctn_stitch_frame(None, p, p, None) == ARG
    assert lib.ctn_stitch_plan(None, p, p, p, p, p, p, 1 << 16, None) == ARG
    assert lib.ctn_stitch_ola(None, p, p, p, p, None) == ARG


def test_capi_rejects_null_pointers_and_short_workspace(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.addressof(buf)
    r = ctypes.byref(_d())
    need = lib.ctn_stitch_workspace_bytes(r)
    assert lib.ctn_stitch_frame(r, None, p, None) == ARG
    assert lib.ctn_stitch_frame(r, p, None, None) == ARG
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert lib.ctn_stitch_plan(r, *args, p, need, None) == ARG
        assert b"null" in lib.ctn_last_error()
    assert lib.ctn_stitch_plan(r, p, p, p, p, p, None, need, None) == ARG
    assert lib.ctn_stitch_plan(r, p, p, p, p, p, p, need - 1, None) == ARG
    assert b"workspace" in lib.ctn_last_error()
    assert lib.ctn_stitch_plan(r, p, p, p, p, p, p, 0, None) == ARG
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert lib.ctn_stitch_ola(r, *args, None) == ARG
    assert lib.ctn_stitch_plan(r, p + 2, p, p, p, p, p, need, None) == ARG      # misaligned P
    assert b"aligned" in lib.ctn_last_error()
