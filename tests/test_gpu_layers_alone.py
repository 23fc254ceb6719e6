"""The stand-alone layer kernels alone (ctn_layers.hip's 14 kernels behind ctn_layernorm_*,
ctn_prelu_*, ctn_depthwise_*, ctn_mask_*) and, through them, the reduction plumbing of
ctn_reduce.hip (the three stats_finalize_* variants, slab_reduce_kernel) against an fp64
restatement, element by element.

ctn_ops.LayerNormFn / PReLUFn / DepthwiseFn / MaskFn run directly on row tensors [M*Kp, C];
gy is handed to backward() as rows too, so the test owns the padded rows of both.  The
oracle (tests/layers_cases.py, checked without a GPU by tests/test_layers_oracle.py) is
plain torch in float64 on the CPU with autograd: conv_tasnet.py:307-355 for gLN / cLN,
F.prelu, conv1d(groups=C) + chomp, relu / softmax over the speakers.  Compared per element:
y, gx, every parameter gradient and, for the norms, the saved stats (mean, rstd; cLN on the
valid rows).  Padded rows (K <= k < Kp) of y and gx must be exactly zero.

What the shapes pin (LY_RB = 64 rows per partial block, Kp = ceil(K/128)*128, nblk = M*Kp/64,
gLN nb = ceil(K/64); launch_stats_finalize: thread for nparts < 2, tile for 2..7 with 64
groups per workgroup, block from 8; slab_reduce: four waves start at part q = w and unroll
32 parts per step while q + 28 < q1, vec4 when n % 4 == 0 and pstride % 4 == 0; ew_grid
caps at 4096 x 256 threads):

    norms, C = 24, M = 2, K = 1 63 64 65 128 129 448 449 513
                         nb = 1 1 1 2 2 3 7 8 9: all three finalize variants, both sides of
                         each switch, a last row block of one row (65, 129, 449, 513)
    norms (65, 65, 8)    tile finalize, two tiles, the second with one group
    norms (257, 10, 8)   thread finalize, two workgroups, the second with one live thread
    norms, prelu (M, 100, 24), M = 1 15 16 17 33
                         2 30 32 34 66 parts into slab_reduce: two waves idle; the unrolled
                         loop in two waves only; exactly on the unroll; past it; past one
                         64-part slice on the single-pass fallback (these entries pass no scratch)
    norms (3, 300, C), C = 1 6 7 24 64 65 130
                         scalar / vec4 slab_reduce, fewer channels than lanes, three lane
                         strides in the cLN wave-per-row kernels
    norms, prelu (9, 1000, 128)
                         1.18 M elements: a second grid-stride trip in ln_apply / ln_dx / prelu_fwd
    prelu (3, 300, C), C = 24 7, alpha = -0.5 0 0.25 1.5, 5 % of the inputs exactly 0 (slope
                         alpha there: torch's convention, prelu_dx's comment).  PReLU's
                         contract is zero padded rows on input; its kernels do not test k < K
    depthwise (P, dil, causal) = (3,1,0) (3,1,1) (3,4,0) (3,128,0) (3,128,1) (1,1,0) (2,1,1)
                         (2,3,1) (5,2,0) at (3, 300) and at (2, 128), where no padded row
                         lies between the utterances and only the kernels' own kk < K keeps a
                         tap off the neighbour; K = 100 with dil = 128 (every tap but one
                         outside); C = 7 8 64, C*P = 21 scalar, 24 and 192 vec4
    mask S = 1 2 3 5, N = 24 64, relu and softmax: rows at +80, -80, +-80 and +-100 by speaker,
                         -100, exact ties, inputs exactly 0 (exp(80) still fits fp32, so the
                         +-100 rows are what a softmax without the max subtraction fails on)

Inputs of the norms carry a per-channel offset of 1.5 to 2.5 standard deviations, one sign
per case, so var = E[x^2] - mean^2 is a real subtraction (median |mean|/std over the groups
>= 1, asserted on the oracle).

fp32 bounds per element, the project's (test_gpu_bn_block.py): y rtol 1e-4 atol 1e-4; gx
rtol 1e-4 atol 2e-4; parameter gradients rtol 1e-3 atol 1e-4*max|ref| + 1e-5; stats rtol 1e-4
atol 1e-5.  bf16 (one case per op at (3, 300) and (2, 129), inputs rounded to bf16 first):
a stored bf16 element within 2^-8*|ref| + the fp32 atol; fp32 parameter gradients and stats
keep the fp32 bounds.  Poisoned padding (+-1e4 in the padded rows of x / score and gy):
valid rows of every output, the stats and every parameter gradient bit-identical to the
zero-padded run, padded output rows still exactly zero ("excluded from every
statistic and every weight-gradient sum").  One backward per op twice: bitwise equal.

Measured on MI355X, worst error / bound per op over all of its cases:

    fp32      y        gx       parameter gradients      stats
    gLN       0.0017   0.0012   gamma 0.0013 beta 0.0014 0.0006
    cLN       0.0040   0.019    gamma 0.0017 beta 0.0012 0.0006
    PReLU     0.0005   0.0004   alpha 0.0008
    depthwise 0.0023   0.0012   w 0.0026
    softmax   0.0011   0.0029   (row sums: 0.40 of S * 2^-23)
    relu      0        0
    bf16      y        gx       parameter gradients / stats as in fp32 (<= 0.0007)
    gLN cLN depthwise softmax   0.91 - 0.97 (PReLU with alpha = 0.25 and relu: 0, exact)

The bf16 figures sit at their bound because of what the bound is: bf16 keeps 8 significant
bits, so one round to nearest is off by up to 2^-8 of the lower end of its binade, and
2^-8 |ref| is met with equality by correct rounding alone (0.97 over a few thousand elements
is the element nearest a power of two); the arithmetic in front of the store contributes
the fp32 figures above, which the added fp32 atol covers a hundred times over.

Found with cLN at C = 1 (gx exactly 0: one channel is its own mean): ln_dx_kernel returned
gx = +-1e-3, 5.0 x its bound, where fp32 torch returns 0.  The build disables packed fp32,
and the compiler then fused g*gamma - mean(g*gamma) into one fma, which keeps the product's
rounding residual (up to 2^-24 |g gamma|) that the separately rounded mean does not have;
a constant row's rstd = 1/sqrt(eps) = 1e4 multiplies it.  ln_dx_kernel now forbids the
contraction (gx at C = 1 is exactly 0 again; no other case moved by more than 0.002 of its
bound).

Not reached from here, and left to the TemporalBlock driver's tests rather than to a test
hook in the C ABI: the cLN tile finalize at G >= 8192 groups, and slab_reduce's two-pass
slice path (it needs scratch, which these entries do not pass).
"""
import pytest
import torch

import layers_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run_hip(case, bf16=False, poison=False):
    """The case through the autograd Function of its op -> {name: fp32 CPU tensor} shaped as
    the oracle's."""
    import ctn_lib as L
    import ctn_ops as ops
    op, M, K = case[:3]
    inp = C.make_inputs(case, bf16, poison)
    dt = torch.bfloat16 if bf16 else torch.float32
    fr = ops.Frames.of(M, K)
    Kp, ch = fr.Kp, C.channels(case)
    assert Kp == C.padded(K)
    x = inp["x"].to(DEV, dt).reshape(M * Kp, ch).requires_grad_(True)
    gy = inp["gy"].to(DEV, dt).reshape(M * Kp, ch)
    par = {n: v.to(DEV).requires_grad_(True) for n, v in inp.items() if n not in ("x", "gy")}
    out = {}
    if op in C.NORMS:
        y = ops.LayerNormFn.apply(x, fr, L.NORM_GLN if op == "gLN" else L.NORM_CLN, par["gamma"], par["beta"])
        stats = y.grad_fn.saved_tensors[2].detach().clone().cpu()
        out["stats"] = stats if op == "gLN" else stats.view(M, Kp, 2)[:, :K]
    elif op == "prelu":
        y = ops.PReLUFn.apply(x, fr, par["alpha"])
    elif op == "dw":
        y = ops.DepthwiseFn.apply(x, fr, (case[4], case[5], bool(case[6])), par["w"])
    else:
        y = ops.MaskFn.apply(x, fr, case[4], L.MASK_RELU if op == "relu" else L.MASK_SOFTMAX)
    assert y.dtype == dt and y.shape == x.shape
    y.backward(gy)
    assert x.grad.dtype == dt
    out["y"] = y.detach().float().cpu().view(M, Kp, ch)
    out["gx"] = x.grad.float().cpu().view(M, Kp, ch)
    for n, p in par.items():
        assert p.grad.dtype == torch.float32
        out["g" + n] = p.grad.cpu()
    # padded frame rows of the output and of the data gradient are exactly zero
    for n in ("y", "gx"):
        assert torch.count_nonzero(out[n][:, K:]) == 0, (C.case_id(case), n)
    return out


def check(case, bf16=False):
    ref, cond = C.reference(case, bf16)
    if not bf16:
        C.check_conditioning(case, cond)
    got = run_hip(case, bf16)
    assert sorted(got) == sorted(ref)
    r = C.ratios(got, ref, bf16)
    C.show(case, "bf16" if bf16 else "fp32", r)
    assert max(r.values()) <= 1.0, (C.case_id(case), r)
    return got, ref


@pytest.mark.parametrize("case", C.LN_CASES, ids=C.case_id)
def test_layer_norm_f32(case):
    check(case)


@pytest.mark.parametrize("case", C.PRELU_CASES, ids=C.case_id)
def test_prelu_f32(case):
    got, ref = check(case)
    if case[4] == 0.0:   # alpha = 0: a plain relu, to the bit
        assert torch.equal(got["y"], ref["y"].float())


@pytest.mark.parametrize("case", C.DW_CASES, ids=C.case_id)
def test_depthwise_f32(case):
    check(case)


@pytest.mark.parametrize("P,dil", C.DW_UNSUPPORTED)
def test_depthwise_rejects_odd_noncausal_padding(P, dil):
    """Non-causal with (P - 1) * dil odd: the reference's output is not K frames long; the
    library says so instead of computing something (tests/test_layers_oracle.py: before it
    touches the device)."""
    import ctn_lib as L
    import ctn_ops as ops
    fr = ops.Frames.of(2, 128)
    x = torch.randn(2 * fr.Kp, 8, device=DEV)
    w = torch.randn(8, 1, P, device=DEV)
    with pytest.raises(L.CtnLibraryError, match="status 2.*odd"):
        ops.DepthwiseFn.apply(x, fr, (P, dil, False), w)
    y = ops.DepthwiseFn.apply(x, fr, (P, dil, True), w)      # the causal call is fine
    assert y.shape == x.shape


@pytest.mark.parametrize("case", C.MASK_CASES, ids=C.case_id)
def test_mask_f32(case):
    got, ref = check(case)
    kind, M, K, N, S = case
    y, gx = got["y"][:, :K].double().view(M, K, S, N), got["gx"][:, :K]
    if kind == "softmax":
        # z = fl(sum of S terms) is off by at most (S - 1) 2^-24 relative and each of the S
        # quotients by 2^-24, so the row sum is within S 2^-24 of 1; a factor two of slack
        err = float((y.sum(2) - 1.0).abs().max())
        print("RATIO", C.case_id(case), "softmax-sum", f"sum={err / (S * 2.0 ** -23):.3g}")
        assert err <= S * 2.0 ** -23, err
        if S == 1:
            assert bool((y == 1.0).all()) and torch.count_nonzero(gx) == 0
    else:
        s = C.make_inputs(case)["x"][:, :K]
        assert int((s == 0).sum()) > 0
        assert torch.count_nonzero(got["y"][:, :K][s <= 0]) == 0 and torch.count_nonzero(gx[s <= 0]) == 0
        assert torch.equal(got["y"][:, :K][s > 0], s[s > 0])


@pytest.mark.parametrize("case", C.POISON_CASES, ids=C.case_id)
def test_poisoned_padding_reaches_nothing(case):
    K = case[2]
    clean, dirty = run_hip(case), run_hip(case, poison=True)    # run_hip: padded output rows are zero
    assert bool((C.make_inputs(case, poison=True)["x"][:, K:].abs() == C.POISON).all())
    for n in clean:
        a, b = clean[n], dirty[n]
        assert torch.equal(a, b), (C.case_id(case), n, int((a != b).sum()), float((a - b).abs().max()))


@pytest.mark.parametrize("case", C.BF16_CASES, ids=C.case_id)
def test_layers_bf16(case):
    check(case, bf16=True)


@pytest.mark.parametrize("case", C.DETERMINISM_CASES, ids=C.case_id)
def test_backward_is_deterministic(case):
    a, b = run_hip(case), run_hip(case)
    for n in a:
        assert torch.equal(a[n], b[n]), (C.case_id(case), n)
