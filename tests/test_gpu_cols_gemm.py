"""The column GEMM (gemm_cols_kernel in ctn_gemm.hip: 128 x 128 output tiles, split-k over
row chunks, two k-split groups per workgroup, fp32 partials summed by slab_reduce) that
computes the first 1x1 conv's weight gradient dW1 = gh1^T . x in the block backward, checked
through the public 1x1 conv layer (ctn_conv1x1_backward: dW = gy^T . x, the same GemmCols
shape C=256 -> 512): against an fp32 matmul of the same bf16 operands and run to run
bitwise; and, with integer operands whose sums are exact in fp32, for EQUALITY with an fp64
matmul at the kernel's own chunk and group edges.  Padded frame rows contribute nothing.
GPU only."""
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


# Geometry (ctn_gemm.hip): P x Q = 512 x 256 is 4 x 2 tiles of CBP x CBQ = 128 x 128, so
# gemm_cols_chunks asks for 256 / 8 = 32 chunks, capped at ceil(rows / (CKS * CKR * 4)) =
# ceil(rows / 256); a chunk is ceil(rows / chunks) rows rounded up to CKS * CKR = 64, and
# its CKS = 2 groups take half each in k-steps of CKR = 32 rows.
#   (32, 3199): 102400 rows, 32 chunks of exactly 3200 = 50 steps per group (on the boundary:
#               a chunk per utterance);
#   (4, 3199):  12800 rows, 32 chunks of 448: chunk 28 holds the last 256 rows (7 + 1 steps)
#               and chunks 29-31 are empty (all-zero partials);
#   (3, 1000):  3072 rows, the cap gives 12 chunks of exactly 256 (on the boundary).
@pytest.mark.parametrize("M,K", [(4, 3199), (32, 3199), (3, 1000)])
def test_cols_gemm_matches_fp32(M, K):
    import ctn_ops as ops
    fr = ops.Frames.of(M, K)
    g = torch.Generator(device=DEV).manual_seed(M * 7 + K)
    x = torch.randn(fr.rows, 256, device=DEV, generator=g).to(torch.bfloat16)
    gy = torch.randn(fr.rows, 512, device=DEV, generator=g).to(torch.bfloat16)
    pad = torch.arange(fr.rows, device=DEV) % fr.Kp >= K      # padded frames are zero rows
    x[pad] = 0
    gy[pad] = 0
    ref = gy.float().t() @ x.float()                           # [512][256]
    a = _dw(x, gy, fr, 512)
    b = _dw(x, gy, fr, 512)
    assert torch.equal(a, b), "run-to-run"
    e = float((a - ref).norm() / ref.norm())
    assert e < 1e-5, e


# The kernel's own edges.  K = 100: Kp = 128, so rows = 128 M and the cap ceil(rows / 256)
# sets the chunk count; every chunk is 256 rows (4 k-steps per group):
#   M = 1:  128 rows, 1 chunk of 128 (2 steps per group);
#   M = 16: 2048 rows, exactly 8 chunks (on the boundary);
#   M = 15, 17, 33: 8, 9, 17 chunks whose last holds 128 rows: group 0 runs 4 steps and
#           group 1 none;
#   (3, 300): Kp = 384, 1152 rows, 5 chunks, the last again half empty, with a band of
#           padded rows inside every utterance.
@pytest.mark.parametrize("M,K", [(1, 100), (15, 100), (16, 100), (17, 100), (33, 100), (3, 300)])
def test_cols_gemm_integer_exact(M, K):
    """x and gy from {-1, 0, 1}: every product and partial sum is an exact fp32 integer, so
    neither the chunks, the k-split groups nor the slab reduction may change a bit: dW
    EQUALS the fp64 matmul."""
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
    a = _dw(xs, gys, fr, 512)
    b = _dw(xs, gys, fr, 512)
    assert torch.equal(a, b), "run-to-run"
    bad = a.double() != ref
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())
