"""The wave-specialised column GEMM (ctn_dual_ws.hip, COLS mode: memory + column waves
only, plain bf16 operands, transposed partials; opt-in, CTN_COLS_WS=1) that can compute
the first 1x1 conv's weight gradient dW1 = gh1^T . x in the block backward, checked through the public 1x1
conv layer (ctn_conv1x1_backward: dW = gy^T . x, the same GemmCols shape C=256 -> 512):
against an fp32 matmul of the same bf16 operands, against the tiled column kernel
(CTN_COLS_WS=0), and run to run bitwise; and, with integer operands whose sums are exact
in fp32, for EQUALITY with an fp64 matmul and with the tiled kernel at the kernel's own
tile and range edges.  Padded frame rows contribute nothing.  GPU only."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dw(x, gy, fr, cout):
    import ctn_ops as ops
    w = torch.nn.Parameter(torch.randn(cout, x.shape[1], 1, device=DEV) * 0.05)
    xr = x.clone().requires_grad_(True)
    y = ops.Conv1x1Fn.apply(xr, fr, w)
    y.backward(gy)
    torch.cuda.synchronize()
    return w.grad.detach().reshape(cout, -1).clone()


@pytest.mark.parametrize("M,K", [(4, 3199), (32, 3199), (3, 1000)])
def test_cols_ws_matches_fp32_and_tiled_kernel(M, K, monkeypatch):
    import ctn_ops as ops
    fr = ops.Frames.of(M, K)
    g = torch.Generator(device=DEV).manual_seed(M * 7 + K)
    x = torch.randn(fr.rows, 256, device=DEV, generator=g).to(torch.bfloat16)
    gy = torch.randn(fr.rows, 512, device=DEV, generator=g).to(torch.bfloat16)
    pad = torch.arange(fr.rows, device=DEV) % fr.Kp >= K      # padded frames are zero rows
    x[pad] = 0
    gy[pad] = 0
    ref = gy.float().t() @ x.float()                           # [512][256]
    monkeypatch.setenv("CTN_COLS_WS", "1")
    a = _dw(x, gy, fr, 512)
    b = _dw(x, gy, fr, 512)
    assert torch.equal(a, b), "run-to-run"
    e = float((a - ref).norm() / ref.norm())
    assert e < 1e-5, e
    monkeypatch.setenv("CTN_COLS_WS", "0")
    c = _dw(x, gy, fr, 512)
    e2 = float((a - c).norm() / c.norm())
    assert e2 < 1e-5, e2


# The kernel's own edges: 32-row tiles over min(tiles, 64) row ranges for P = 512 (four
# 128-channel slices of a 256-workgroup grid).  K = 100: Kp = 128, 4 M tiles: M = 1 -> 4
# ranges of one tile, 15 -> 60, 16 -> exactly 64, 17 -> 68 tiles (1-2 per range), 33 -> 132
# (2-3 per range); (3, 300): Kp = 384, 36 ranges, a padding band inside the grid.
@pytest.mark.parametrize("M,K", [(1, 100), (15, 100), (16, 100), (17, 100), (33, 100), (3, 300)])
def test_cols_ws_integer_exact(M, K, monkeypatch):
    """x and gy from {-1, 0, 1}: every product and partial sum is an exact fp32 integer, so
    neither the row ranges nor the slab reduction may change a bit: dW EQUALS the fp64
    matmul and the tiled kernel's result."""
    import ctn_ops as ops
    fr = ops.Frames.of(M, K)
    g = torch.Generator().manual_seed(M * 7 + K)
    x = torch.randint(-1, 2, (fr.rows, 256), generator=g, dtype=torch.int8)
    gy = torch.randint(-1, 2, (fr.rows, 512), generator=g, dtype=torch.int8)
    pad = torch.arange(fr.rows) % fr.Kp >= K                   # padded frames are zero rows
    x[pad] = 0
    gy[pad] = 0
    x, gy = x.to(DEV), gy.to(DEV)
    ref = gy.double().t() @ x.double()                         # [512][256], |ref| < 2^24
    xs, gys = x.to(torch.bfloat16), gy.to(torch.bfloat16)
    monkeypatch.setenv("CTN_COLS_WS", "1")
    a = _dw(xs, gys, fr, 512)
    b = _dw(xs, gys, fr, 512)
    assert torch.equal(a, b), "run-to-run"
    bad = a.double() != ref
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())
    monkeypatch.setenv("CTN_COLS_WS", "0")
    c = _dw(xs, gys, fr, 512)
    assert torch.equal(a, c), "wave-specialised vs tiled kernel"
