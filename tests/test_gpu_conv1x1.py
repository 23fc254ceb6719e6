"""The 1x1-conv GEMMs on their own, element by element, at their tile and grid edges.

The public layer ctn_conv1x1_forward/backward (ops.Conv1x1Fn) reaches, in the plain-operand
plain-store form, the weight-stationary row GEMM (ctn_gemm_ws.hip), the tiled row GEMM and
the tiled column GEMM (ctn_gemm.hip).  Every other test runs these kernels inside a
TemporalBlock or the model and compares by relative L2 over whole utterances, which one
dropped, duplicated or misplaced tile cannot move.  Here the reference is an fp64 torch
matmul of exactly the operands the kernel sees (CTN_GEMM_WS / CTN_WS_1536 are cached in the
library and cannot serve as in-process A/B oracles).  Inputs come from a seeded CPU
generator, are rounded to the storage type, and their padded frame rows are zeroed (the
library's contract: padded rows are zero).

  (a) test_int_exact       x, w, gy in {-1, 0, 1}: every product and partial sum is an exact
                           fp32 integer, so accumulation order, split-K chunks and the slab
                           reduction cannot change the result: y, gx, gw must EQUAL the fp64
                           reference, twice (run to run).  bf16 stores are exact for
                           |v| <= 256 only: a condition that is asserted, not a tolerance
                           (sigma = sqrt(Kred * 4/9) <= 26.2 at Kred <= 1536; if a seed ever
                           violates it, thin the alphabet, never relax the comparison).
  (b) test_gauss_elementwise  N(0,1) x and gy, N(0, 0.05^2) w, rounded to bf16; per element
                           |y - ref| <= 2^-8 |ref| + Kred 2^-23 S,  S = |x| . |w|^T in fp64
                           (fp32 storage: the second term alone); gx likewise with
                           Kred = cout; gw by the project's bound (test_gpu_cols_gemm.py):
                           relative L2 < 1e-5 against the fp32 matmul of the same operands.
  (c) test_guard_bands     y and gx as views into larger buffers between 64 sentinel rows:
                           the clamped look-ahead tiles past a range's end are "never
                           stored"; the sentinels must survive and every row between them
                           must have been written.
  (d) test_int_preconditions_cpu   (no GPU) the inputs of (a) rebuilt from the same seeds:
                           the bf16 round trip is the identity and max |ref| <= 256 for y and
                           gx of EVERY bf16 case of (a) (fp64 matmul on the CPU; nothing is
                           left to the GPU-side assertion, which (a) repeats anyway).

The bounds of (b) are derived, not measured.  The kernels multiply bf16 (or fp32) operands
exactly into fp32 and accumulate Kred terms in fp32 in some order (MFMA blocks, k-steps):
for any order the accumulated value v satisfies |v - ref| <= gamma(Kred - 1) S with
gamma(n) = n u / (1 - n u) and u = 2^-24 (Higham, Accuracy and Stability, 3.1), which is
below Kred 2^-24 S (1 + 1e-4) here; Kred 2^-23 S is twice that worst case.  A bf16 store
rounds v to nearest: |y - v| <= 2^-8 |v| <= 2^-8 |ref| + 2^-8 |v - ref|, whose first term is
the first term of the bound (one bf16 ulp of the result) and whose remainder is far inside
the factor two of the second.

Row geometries.  With K <= 128 the padded length is Kp = 128 and rows = 128 M: 4 M tiles
of 32 rows, 8 M tiles of 16 rows.  A kernel's grid is min(tiles, cap) row ranges; range r
takes tiles [tiles r / ranges, tiles (r + 1) / ranges).  Constants the table was built for
(test_table_constants_match_the_source pins them): WS_GRID = 256, cap 80 =
(256 / 3) / 8 * 8 for the three-slice 1536-channel form, WS_DR = 6 (the LDS-DMA ring of
the 16-wave forms: 5 tiles in flight in the prologue), 32-row tiles for 512 / 1536 outputs,
16-row tiles and a two-accumulator software pipeline (tile parity) for 256 outputs.

  bf16 forward      kernel               tile cap   M: tiles per range
  256 -> 512        ws 16 waves, ring     32  256   1, 3, 63: 1 (4, 12, 252 ranges) | 64: 1 (256) |
                                                    65: 1-2 | 128: 2 | 161: 2-3 | 320: 5 | 384: 6 |
                                                    400: 6-7 | 448: 7 | 520: 8-9
  256 -> 1536       ws 3 slices, ring     32   80   1, 3, 5, 19: 1 (4, 12, 20, 76 ranges: nr % 8 != 0,
                                                    the fallback slice mapping) | 20: 1 (80 ranges,
                                                    nr % 8 == 0 from here on) | 21: 1-2 | 40: 2 |
                                                    50: 2-3 | 100: 5 | 120: 6 | 130: 6-7 | 140: 7 |
                                                    170: 8-9
  512 -> 256        ws 8 waves            16  256   1, 31: 1 (8, 248 ranges) | 32: 1 (256) | 33: 1-2 |
  256 -> 256        ws 8 waves            16  256   64: 2 | 81: 2-3 | 192: 6 | 200: 6-7 | 224: 7 |
                                                    260: 8-9                     (both shapes)
  bf16 data gradient (gx = gy . w), same M lists
  of 256 -> 512     ws 8 waves (256<-512) 16  256   1, 3: 1 | 63: 1-2 | 64: 2 | 65: 2-3 | 128: 4 |
                                                    161: 5-6 | 320: 10 | 384: 12 | 400: 12-13 |
                                                    448: 14 | 520: 16-17
  of 512 -> 256     ws 16 waves, ring     32  256   1, 31, 32, 33: 1 | 64: 1 (256) | 81: 1-2 | 192: 3 |
                                                    200: 3-4 | 224: 3-4 | 260: 4-5
  of 256 -> 256     as its forward
  of 256 -> 1536    tiled rows kernel (64-row tiles, 128-column tiles), 1536-long reduction
  weight gradient   tiled column kernel (128 x 128 tiles, split-K chunks, slab reduction)
  tail shapes 8 -> 8, 96 -> 160, 264 -> 136 and every fp32 case: the tiled kernels
  (column-tile tails; the P/Q tails of the column GEMM), M = 1, 3, 33, 65.

K: 1 (with M = 1 only), then 97, 100, 127, 128: the padding boundary in the middle of a
32-row tile, at row 4 of a tile, on a tile's last row, and absent.  M = 1 runs at all of
them; the other M take them in turn (every M list meets every K).  Two Kp > 128 cases per
weight-stationary shape, (M, K) = (5, 129) and (3, 300): ranges that straddle utterances
and a padding band in the middle of a range.  A change to WS_GRID, WS_DR, the
tile rows or the slice counts moves the rows of this table: rebuild the M lists from them
(M such that tiles = cap - 1 tile's worth, cap, cap + 1, and 5, 6, 6-7, 7 tiles per range).
"""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

DEV = "cuda"
gpu = pytest.mark.gpu

WS_GRID, WS_GRID_1536, WS_DR = 256, 80, 6     # the constants the table above was built for
KS = (97, 100, 127, 128)
M_512 = (1, 3, 63, 64, 65, 128, 161, 320, 384, 400, 448, 520)
M_1536 = (1, 3, 5, 19, 20, 21, 40, 50, 100, 120, 130, 140, 170)
M_256 = (1, 31, 32, 33, 64, 81, 192, 200, 224, 260)
M_SUB = (1, 3, 33, 65)
LONG = ((5, 129), (3, 300))                    # Kp = 256 and 384
WS_SHAPES = {(256, 512): M_512, (256, 1536): M_1536, (512, 256): M_256, (256, 256): M_256}
TAIL_SHAPES = ((8, 8), (96, 160), (264, 136))
# (b) and (c): first, cap - 1, cap, cap + 1 and largest M of each weight-stationary shape
EDGE_M = {(256, 512): (1, 63, 64, 65, 520), (256, 1536): (1, 19, 20, 21, 170),
          (512, 256): (1, 31, 32, 33, 260), (256, 256): (1, 31, 32, 33, 260)}


def _geoms(ms, extra=()):
    out = [(1, 1)] + [(1, k) for k in KS]
    out += [(m, KS[i % len(KS)]) for i, m in enumerate(m for m in ms if m != 1)]
    return out + list(extra)


def _int_cases():
    """(C, cout, dtype name, M, K) of test (a)."""
    cases = []
    for (c, co), ms in WS_SHAPES.items():
        cases += [(c, co, "bf16", m, k) for m, k in _geoms(ms, LONG)]
    for c, co in TAIL_SHAPES:
        cases += [(c, co, "bf16", m, k) for m, k in _geoms(M_SUB)]
    for c, co in list(WS_SHAPES) + list(TAIL_SHAPES):
        cases += [(c, co, "f32", m, k) for m, k in _geoms(M_SUB)]
    return cases


def _gauss_cases():
    cases = []
    for (c, co), ms in EDGE_M.items():
        cases += [(c, co, "bf16", m, 100) for m in ms]
    for c, co in TAIL_SHAPES:
        cases += [(c, co, "bf16", m, 100) for m in M_SUB]
    for c, co in list(WS_SHAPES) + list(TAIL_SHAPES):
        cases += [(c, co, "f32", m, 100) for m in M_SUB]
    return cases


def _id(case):
    c, co, dt, m, k = case
    return f"{c}to{co}-{dt}-M{m}-K{k}"


def _dtype(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _padded(K):
    return (K + 127) // 128 * 128


def _seed(c, co, m, k):
    return ((c * 4099 + co) * 4099 + m) * 4099 + k


def _zero_pad(t, M, K):
    t.view(M, _padded(K), -1)[:, K:] = 0
    return t


def int_inputs(c, co, m, k):
    """x [rows, C], w [cout, C], gy [rows, cout] from {-1, 0, 1} as fp32 on the CPU, padded
    frame rows zero; the same tensors for the same arguments everywhere."""
    g = torch.Generator().manual_seed(_seed(c, co, m, k))
    rows = m * _padded(k)
    x = _zero_pad(torch.randint(-1, 2, (rows, c), generator=g, dtype=torch.int8), m, k)
    w = torch.randint(-1, 2, (co, c), generator=g, dtype=torch.int8)
    gy = _zero_pad(torch.randint(-1, 2, (rows, co), generator=g, dtype=torch.int8), m, k)
    return x.float(), w.float(), gy.float()


def gauss_inputs(c, co, m, k):
    """N(0,1) x and gy, N(0, 0.05^2) w, rounded to bf16 (held as fp32), padded rows zero."""
    g = torch.Generator().manual_seed(_seed(c, co, m, k) + 1)
    rows = m * _padded(k)
    x = _zero_pad(torch.randn(rows, c, generator=g), m, k)
    w = torch.randn(co, c, generator=g) * 0.05
    gy = _zero_pad(torch.randn(rows, co, generator=g), m, k)
    return tuple(t.bfloat16().float() for t in (x, w, gy))


def tiles_per_range(rows, tile, cap):
    """(ranges, fewest, most tiles of a range) of the weight-stationary partition."""
    nt = rows // tile
    nr = min(nt, cap)
    n = [nt * (r + 1) // nr - nt * r // nr for r in range(nr)]
    return nr, min(n), max(n)


# ----------------------------------------------------------------------------
# CPU: the table's constants, its rows, and the preconditions of the exact test
# ----------------------------------------------------------------------------
def test_table_constants_match_the_source():
    src = open(os.path.join(ROOT, "conv-tasnet_amd", "csrc", "ctn_gemm_ws.hip")).read()
    assert int(re.search(r"constexpr int WS_WAVES = 8, WS_TM = 16, WS_GRID = (\d+);", src).group(1)) == WS_GRID
    assert int(re.search(r"constexpr int WS_DR = (\d+);", src).group(1)) == WS_DR
    assert (WS_GRID // 3) // 8 * 8 == WS_GRID_1536
    assert "(WS_GRID / 3) / 8 * 8" in src and "constexpr int WS_WAVES = 8, WS_TM = 16" in src


def test_geometry_lists_cover_the_edges():
    """The M lists hit, per kernel configuration: grids of a few tiles, cap - 1 tile's worth,
    exactly the cap, one utterance over it, and 5 (ring prologue), 6 (ring depth), 6-7, 7 and
    more tiles per range; the 1536 form both slice mappings."""
    def per(ms, tile, cap):
        return {m: tiles_per_range(128 * m, tile, cap) for m in ms}
    for ms, tile, cap, at_cap in ((M_512, 32, WS_GRID, 64), (M_1536, 32, WS_GRID_1536, 20), (M_256, 16, WS_GRID, 32)):
        t = per(ms, tile, cap)
        assert t[1][0] < 16 and t[1][1:] == (1, 1)
        assert t[at_cap] == (cap, 1, 1)
        below, above = ms[ms.index(at_cap) - 1], ms[ms.index(at_cap) + 1]
        assert cap - 128 // tile <= t[below][0] < cap and t[above] == (cap, 1, 2)
        spans = {v[1:] for v in t.values()}
        assert {(2, 2), (2, 3), (WS_DR, WS_DR), (WS_DR, WS_DR + 1), (WS_DR + 1, WS_DR + 1), (8, 9)} <= spans
        if tile == 32:
            assert (WS_DR - 1, WS_DR - 1) in spans
    nr = [tiles_per_range(128 * m, 32, WS_GRID_1536)[0] for m in M_1536]
    assert {4, 12, 20, 76} <= {n for n in nr if n % 8} and WS_GRID_1536 in nr
    assert len({_id(c) for c in _int_cases()}) == len(_int_cases())


@pytest.mark.parametrize("shape", list(WS_SHAPES) + list(TAIL_SHAPES), ids=lambda s: f"{s[0]}to{s[1]}")
def test_int_preconditions_cpu(shape):
    """Every bf16 case of (a): inputs survive the bf16 round trip, |y| and |gx| <= 256."""
    c, co = shape
    for _, _, _, m, k in [cs for cs in _int_cases() if cs[:3] == (c, co, "bf16")]:
        x, w, gy = int_inputs(c, co, m, k)
        for t in (x, w, gy):
            assert torch.equal(t.bfloat16().float(), t)
        assert int(x.view(m, _padded(k), c)[:, k:].count_nonzero()) == 0
        y = x.double() @ w.double().t()
        assert float(y.abs().max()) <= 256, (m, k)
        del y
        gx = gy.double() @ w.double()
        assert float(gx.abs().max()) <= 256, (m, k)


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def _conv(x, w, gy, fr):
    import ctn_ops as ops
    xr = x.clone().requires_grad_(True)
    wp = w.clone().unsqueeze(-1).requires_grad_(True)      # [cout, C, 1] fp32 parameter
    y = ops.Conv1x1Fn.apply(xr, fr, wp)
    y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xr.grad, wp.grad.reshape(w.shape)


def _assert_exact(got, ref, what):
    """got == ref everywhere, or a message that names the wrong rows and columns."""
    bad = got.double() != ref
    if not bool(bad.any()):
        return
    rows = bad.any(1).nonzero().flatten().tolist()
    cols = bad.any(0).nonzero().flatten().tolist()
    r, c = rows[0], int(bad[rows[0]].nonzero()[0])
    tiles = "" if what == "gw" else f", 16-row tiles {rows[0] // 16}..{rows[-1] // 16}"
    raise AssertionError(
        f"{what}: {int(bad.sum())} wrong elements; rows {rows[0]}..{rows[-1]} ({len(rows)} rows{tiles}), "
        f"columns {cols[0]}..{cols[-1]} ({len(cols)} columns); "
        f"first at ({r}, {c}): got {float(got[r, c])}, expected {float(ref[r, c])}")


def _pad_rows(t, fr):
    return t.view(fr.M, fr.Kp, -1)[:, fr.K:]


@gpu
@pytest.mark.parametrize("case", _int_cases(), ids=_id)
def test_int_exact(case):
    import ctn_ops as ops
    c, co, dn, m, k = case
    dt = _dtype(dn)
    fr = ops.Frames.of(m, k)
    assert fr.Kp == _padded(k)
    x, w, gy = (t.to(DEV) for t in int_inputs(c, co, m, k))
    ref_y = x.double() @ w.double().t()
    ref_gx = gy.double() @ w.double()
    ref_gw = gy.double().t() @ x.double()
    if dt == torch.bfloat16:      # the condition under which a bf16 store is exact
        assert float(ref_y.abs().max()) <= 256 and float(ref_gx.abs().max()) <= 256
    assert float(ref_gw.abs().max()) < 2 ** 24
    xs, gys = x.to(dt), gy.to(dt)
    y, gx, gw = _conv(xs, w, gys, fr)
    assert y.dtype == dt and gx.dtype == dt and gw.dtype == torch.float32
    _assert_exact(y, ref_y, "y")
    _assert_exact(gx, ref_gx, "gx")
    _assert_exact(gw, ref_gw, "gw")
    assert int(_pad_rows(y, fr).count_nonzero()) == 0 and int(_pad_rows(gx, fr).count_nonzero()) == 0
    y2, gx2, gw2 = _conv(xs, w, gys, fr)
    assert torch.equal(y, y2) and torch.equal(gx, gx2) and torch.equal(gw, gw2), "run to run"


@gpu
@pytest.mark.parametrize("case", _gauss_cases(), ids=_id)
def test_gauss_elementwise(case):
    import ctn_ops as ops
    c, co, dn, m, k = case
    dt = _dtype(dn)
    fr = ops.Frames.of(m, k)
    x, w, gy = (t.to(DEV) for t in gauss_inputs(c, co, m, k))
    y, gx, gw = _conv(x.to(dt), w, gy.to(dt), fr)
    store = 2.0 ** -8 if dt == torch.bfloat16 else 0.0

    def worst(got, a, b, kred):       # max over elements of |got - a.b| / bound
        a, b = a.double(), b.double()
        ref = a @ b
        bound = store * ref.abs() + kred * 2.0 ** -23 * (a.abs() @ b.abs())
        err = (got.double() - ref).abs()
        assert bool(torch.isfinite(got).all())
        ok = err <= bound             # 0 <= 0 on the padded rows
        return float((err / bound.clamp_min(1e-300)).max()), bool(ok.all())

    ry, oky = worst(y, x, w.t(), c)
    rgx, okgx = worst(gx, gy, w, co)
    ref32 = gy.t() @ x                                   # fp32 matmul of the same operands
    egw = float((gw - ref32).norm() / ref32.norm())
    egw64 = float((gw.double() - gy.double().t() @ x.double()).norm() / ref32.double().norm())
    print(f"\nconv1x1 {_id(case)}: worst error/bound y {ry:.3f} gx {rgx:.3f}; "
          f"gw rel L2 {egw:.2e} vs fp32 matmul ({egw64:.2e} vs fp64)")
    assert oky, f"y: worst error/bound {ry}"
    assert okgx, f"gx: worst error/bound {rgx}"
    assert egw < 1e-5, egw
    assert int(_pad_rows(y, fr).count_nonzero()) == 0 and int(_pad_rows(gx, fr).count_nonzero()) == 0


GUARD = 64


def _guarded(rows, ch):
    """A bf16 [GUARD + rows + GUARD, ch] buffer filled with 0x7f7f and its int16 view."""
    buf = torch.empty(rows + 2 * GUARD, ch, dtype=torch.bfloat16, device=DEV)
    bits = buf.view(torch.int16)
    bits.fill_(0x7F7F)
    return buf, bits


def _guards_intact(bits):
    return bool((bits[:GUARD] == 0x7F7F).all()) and bool((bits[-GUARD:] == 0x7F7F).all())


@gpu
@pytest.mark.parametrize("case", [(c, co, "bf16", m, 100) for (c, co), ms in EDGE_M.items()
                                  for m in (ms[0], ms[1], ms[3])], ids=_id)
def test_guard_bands(case):
    import ctn_lib as L
    import ctn_ops as ops
    c, co, _, m, k = case
    lib = L.load()
    fr = ops.Frames.of(m, k)
    x, w, gy = (t.to(DEV) for t in int_inputs(c, co, m, k))
    ref_y = x.double() @ w.double().t()
    ref_gx = gy.double() @ w.double()
    ref_gw = gy.double().t() @ x.double()
    xs, gys, w = x.bfloat16().contiguous(), gy.bfloat16().contiguous(), w.contiguous()
    d = ops.rows_desc(fr, c, torch.bfloat16)

    ybuf, ybits = _guarded(fr.rows, co)
    nb = lib.ctn_conv1x1_workspace_bytes(ctypes.byref(d), co, 0)
    ws = L.workspace(nb, xs.device)
    L.check(lib.ctn_conv1x1_forward(ctypes.byref(d), co, xs.data_ptr(), w.data_ptr(), ybuf[GUARD:].data_ptr(),
                                    ws.data_ptr(), nb, L.stream_handle(xs.device)), "ctn_conv1x1_forward")
    torch.cuda.synchronize()
    assert _guards_intact(ybits), "y: sentinel rows overwritten"
    y = ybuf[GUARD:GUARD + fr.rows]
    _assert_exact(y, ref_y, "y")                          # a row never written keeps 0x7f7f
    assert int(_pad_rows(y, fr).count_nonzero()) == 0

    gbuf, gbits = _guarded(fr.rows, c)
    gw = torch.empty(co, c, dtype=torch.float32, device=DEV)
    nb = lib.ctn_conv1x1_workspace_bytes(ctypes.byref(d), co, 1)
    ws = L.workspace(nb, xs.device)
    L.check(lib.ctn_conv1x1_backward(ctypes.byref(d), co, xs.data_ptr(), w.data_ptr(), gys.data_ptr(),
                                     gbuf[GUARD:].data_ptr(), gw.data_ptr(), ws.data_ptr(), nb,
                                     L.stream_handle(xs.device)), "ctn_conv1x1_backward")
    torch.cuda.synchronize()
    assert _guards_intact(gbits), "gx: sentinel rows overwritten"
    gx = gbuf[GUARD:GUARD + fr.rows]
    _assert_exact(gx, ref_gx, "gx")
    assert int(_pad_rows(gx, fr).count_nonzero()) == 0
    _assert_exact(gw, ref_gw, "gw")
