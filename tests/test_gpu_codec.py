"""The encoder / decoder kernels on their own, element by element, at frame, block and grid edges.

ctn_codec.hip holds eleven kernels (enc_fwd, enc_bwd_rows, frame_outer, dec_fwd, ola_fwd,
dec_bwd, dec_fwd_mfma, dec_bwd_mfma, enc_fwd_mfma, frames_bf16, unpad_cols) behind
ctn_encoder_* / ctn_decoder_* (ops.EncoderFn / ops.DecoderFn).  The other tests reach them at
one small fp32 shape or through the whole model with a relative L2 over whole utterances,
which one dropped, duplicated or misplaced 16-row block, a wrong last frame, a wrong last
basis column or a wrong overlap-add tail cannot move.  Here every reference is plain fp64
torch on the CPU of exactly the operands the kernels see:

  encoder   conv1d(stride = L // 2) -> ReLU -> cLN over N (eps 1e-8) -> bottleneck matmul
  decoder   mask matmul -> relu / softmax over C / identity -> product with w -> basis
            matmul -> overlap-add by index_add -> zero tail
  gradients autograd of the above in fp64

Inputs come from a seeded CPU generator and are rounded to the storage type (activations:
fp32 or bf16; parameters, the mixture and dL/dest are fp32 in the library); padded frame rows
(k >= K) are zero, the library's contract.  CTN_DEC_MFMA, CTN_ENC_MFMA, CTN_DU_COLS and
CTN_DV_COLS are read at every launch: every bf16 case runs as "mfma" (all four on) and as
"valu" (all four off) against the same reference.

  (a) test_int_exact        mixture, U, V, w_rows, mask rows, dL/dw and dL/dest in {-1, 0, 1}:
                            every product and partial sum is an exact fp32 integer, so
                            accumulation order, MFMA blocking, split-K chunks and the slab
                            reduction cannot change a bit.  fp32 outputs (est, gU, gV, gwm)
                            must EQUAL the fp64 reference; bf16 outputs (w_rows, g_w_rows,
                            g_x_last) must equal the reference rounded to bf16 by torch
                            (pk_bf16 is round-to-nearest-even, as torch's cast).  Twice,
                            run to run.  Conditions (asserted, never tolerances): every fp32
                            accumulator < 2^24 (bounded by terms x largest term: |pre| <= L,
                            |frames| <= N, |est| <= 3 N, |gsrc| <= L, |g_w| <= C L,
                            |g_x_last| <= C N L, |gU| <= M K, |gV| <= M K C,
                            |gwm| <= M K L) and every value the kernels round to bf16 BEFORE
                            using it as an operand (src = w act, gpre_bf, xfr, gfr) has
                            |v| <= 256 and survives the bf16 round trip.  The mask-conv path
                            runs with relu and a signed selection matrix Wm (one +-1 per row
                            among B = 8 inputs): score in {-1, 0, 1}, act in {0, 1}.
  (b) test_int_preconditions_cpu   (no GPU) the inputs of (a) rebuilt from their seeds and
                            the conditions above asserted from the fp64 reference.  If a seed
                            ever violates one, thin the alphabet; never relax the comparison.
  (c) test_gauss_*          N(0, 1) data, weights scaled so that scores and pre-activations
                            are O(1), |score| <= 8 (clamped where the score is an input,
                            asserted where the mask conv computes it).  Direct products are
                            bounded per element, composite outputs against a rounding model
                            (below).
  (d) test_guard_bands_and_padding   the C ABI called directly: every output and the
                            workspace (exactly ctn_*_workspace_bytes) between sentinel bands,
                            outputs pre-filled with NaN; sentinels intact, no NaN left (the
                            ABI documents no unwritten rows), padded rows of w_rows, x0,
                            score, g_w_rows and g_x_last exactly zero, est zero from
                            (K - 1) S + L on, cLN statistics of padded rows (0, 1); and the
                            mixture and dL/dest samples past (K - 1) S + L (set to 1000, then
                            to -777) reach no output: all outputs bit-equal.
  (e) test_table_constants_match_the_source   (no GPU) pins the constants the table below is
                            built from.

Bounds of (c): derived, not measured.  u = 2^-8 for bf16 storage, 0 for fp32; S is the same
product taken over absolute values in fp64.  A kernel multiplies its operands exactly into
fp32 and accumulates n terms in fp32 in some order: for any order |v - ref| <= gamma(n) S
with gamma(n) = n 2^-24 / (1 - n 2^-24) (Higham, Accuracy and Stability, 3.1), below
n 2^-24 S (1 + 1e-4) here; n 2^-23 S is twice that.
  encoder w   |w - ref| <= u |ref| + L 2^-23 S, S = |x frames| . |U|^T: L fp32 terms, ReLU is
              1-Lipschitz, one bf16 store (|w - v| <= 2^-8 |v| <= 2^-8 |ref| + 2^-8 |v - ref|,
              the remainder far inside the factor two).
  score       (mask conv, a 1x1 GEMM) |score - ref| <= u |ref| + B 2^-23 S, as test_gpu_conv1x1.
  est         |est - ref| <= (2 u + N 2^-23 + eps_act) S, S = overlap-add of
              (|w| act) . |V|^T over the frames that cover the sample, ref and S formed in
              fp64 from the score the kernel itself stored (so the score's own rounding is
              not charged twice).  One fp32 product w act (2^-24), N terms (gamma(N)), at
              most three overlapping frames (3 2^-24): (N + 4) 2^-24 <= N 2^-23 for N >= 8.
              The matrix-core path rounds src and V to bf16 (2^-9 each, round to nearest):
              (1 + 2^-9)^2 - 1 < 2^-8 <= 2 u; absent in fp32 and on the VALU path.
              eps_act = 0 for identity and relu (exact), 2^-16 for softmax: an ASSUMPTION
              about __expf and the division at arguments in [-16, 0], not a measurement; it
              sits 2^8 below the bf16 term, so it cannot hide a bf16-path error.  (It held on
              an MI355X: the worst fp32 softmax est error was 0.005 of the whole bound.)
  composite   x0, g_x_last, g_w_rows and the weight-type gradients (gU, ggamma0, gbeta0, gwb,
              gwm, gV) pass through several stored-bf16 tensors.  They are bounded against a
              ROUNDING MODEL: the fp64 reference recomputed with every tensor the library
              stores in bf16 rounded to bf16 at that point (w_rows, x0, score, gscore, gcln,
              gpre_bf, xfr, srcb, gfr, the bf16 weight copies, and the bf16 outputs; the cLN
              statistics come from the fp32 values before w_rows is stored, as in enc_fwd):
              rel-L2(kernel, fp64 ref) <= 2 rel-L2(model, fp64 ref) + 1e-5.  The factor 2
              covers the in-register roundings the model does not see (src and V fragments,
              normalised GEMM operands); 1e-5 is the project's fp32 floor
              (test_gpu_layers.py).  In fp32 the model term is zero and 1e-5 stands alone.
              The codec has no PReLU, hence no cancelling scalar sums and no alpha exception.
              (A ReLU gate whose fp64 argument lies within the fp32 accumulation error of
              zero could open on one side only and cost about 1 / sqrt(elements) in fp32; with
              these seeds none does.  If a changed seed meets one, change the seed.)

Geometry table (smallest shapes that reach each edge; rebuild it if a constant moves).
Constants: EN_RPB = 128 rows per encoder workgroup, ROW_TILE = 128 (Kp), matrix-core blocks
of 16 rows in DM_WAVES = 4 waves per workgroup and at most 1024 workgroups (a block with
k0 >= K is skipped), frame_outer chunks of FO_R = 16 rows (8 for 5 <= C <= 8, 4 above) over
at most FO_WGS = 512 workgroups, L <= FO_LMAX = 32, ola_fwd at most 4096 workgroups of 256.
  K    1 (T = L and T = L + S - 1) | 15 one row short of a block | 16 next block wholly
       padded | 17 one valid row in a block | 97 mid-block padding boundary | 127 one short
       of Kp | 128 no padding | 129 Kp = 256 | 300 Kp = 384 (with M = 3: a padding band
       between utterances)
  T    (K - 1) S + L and (K - 1) S + L + S - 1 (the longest tail that adds no frame)
  L    2 (S = 1) | 5 (odd, S = 2: three frames overlap) | 16 (one basis block, Lp = L) |
       20 (the paper's, Lp = 24) | 30 (Lp = 32 != L) | 32 (the maximum, Lp = L: unpad_cols
       skipped, both 16-column blocks full)
  N    8 (one 8-channel group) | 64 (VALU only) | 256, 512 (matrix cores, both templates)
  C    1, 2, 3, 4 (every CM of the matrix-core kernels, at N = 256 and 512) | 5, 8 (CM = 8,
       fo_rows = 8) | 9, 16 (CM = 16, fo_rows = 4); C > 4 runs the VALU kernels in bf16 too
  M    1, 3 | 65 at K = 100: 8320 rows > FO_WGS 16, frame_outer loops | 513 at K = 100,
       N = 256, C = 1: 65 664 rows > 1024 4 16, the persistent matrix-core waves take a
       second iteration | (M, K, C) = (9, 3000, 4), L = 20: M C T = 1 080 360 > 4096 256,
       ola_fwd loops
M = 1 meets every K (L = 20) and every L (K = 97 with both T, K = 1 with the long T) at
N = 256, C = 2; every other axis is walked with the rest at a small default.  Two accepted
configurations nothing had run get one fp32 case each: N = 512, L = 32 (dec_fwd asks for
68 KB and enc_fwd for 72 KB of dynamic LDS) and N = 512, L = 20, C = 16 (dec_fwd: 72 KB):
each must compute the exact result or be refused up front (0 workspace bytes,
CTN_ERR_UNSUPPORTED), never fail from the middle of a call.  (On gfx950 both launch and are
exact.)

What (a) found when it was written: dec_bwd_mfma stored garbage as dL/dscore for the identity
mask, i.e. every bf16 "mfma" case of the standalone decoder failed on g_x_last with est,
g_w_rows and gV exact; fixed in ctn_codec.hip.
"""
import collections
import ctypes
import functools
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

DEV = "cuda"
gpu = pytest.mark.gpu

# the constants the table above was built for (test_table_constants_match_the_source)
EN_RPB, ROW_TILE, DM_WAVES, DM_GRID_CAP = 128, 128, 4, 1024
FO_R, FO_WGS, FO_LMAX, OLA_GRID_CAP = 16, 512, 32, 4096
MASK_RELU, MASK_SOFTMAX, MASK_IDENTITY = 0, 1, 2
ERR_UNSUPPORTED = 2
ENVS = ("CTN_DEC_MFMA", "CTN_ENC_MFMA", "CTN_DU_COLS", "CTN_DV_COLS")

Geo = collections.namedtuple("Geo", "M K tail L N C")   # tail: 1 = T carries S - 1 extra samples

KS = (1, 15, 16, 17, 97, 127, 128, 129, 300)
LS = (2, 5, 16, 20, 30, 32)


def _S(g):
    return g.L // 2


def _T(g):
    return (g.K - 1) * _S(g) + g.L + (g.tail * (_S(g) - 1))


def _padded(K):
    return (K + ROW_TILE - 1) // ROW_TILE * ROW_TILE


def _variants(g, f32=True, bf16=True):
    """(dtype name, variant) of a geometry: the matrix-core variant first, so that it never
    finds a VALU run's results of the same sizes in recycled memory.  Where the matrix-core
    decoder does not apply (N not 256 / 512, or C > 4) "mfma" still switches the encoder's
    dU column GEMM."""
    return ([("bf16", "mfma"), ("bf16", "valu")] if bf16 else []) + ([("f32", "valu")] if f32 else [])


def _std_geoms():
    gs = []
    for k in KS:                                           # every K, both T, M = 1
        gs += [Geo(1, k, t, 20, 256, 2) for t in (0, 1)]
    for l in (l for l in LS if l != 20):                  # every L
        gs += [Geo(1, 97, t, l, 256, 2) for t in ((0, 1) if l // 2 > 1 else (0,))]
        gs += [Geo(1, 1, 1, l, 256, 2)]
    gs += [Geo(3, 300, 1, 20, 256, 2), Geo(5, 129, 0, 20, 256, 2)]   # Kp > 128 with M > 1
    gs += [Geo(3, 100, 1, 20, n, 2) for n in (8, 64, 512)]           # N
    gs += [Geo(3, 100, 1, 32, 512, 2), Geo(2, 17, 0, 16, 512, 2)]    # N = 512 at the L edges
    gs += [Geo(3, 100, 1, 20, 256, c) for c in (1, 3, 4)]            # every CM, both templates
    gs += [Geo(2, 100, 0, 30, 512, c) for c in (1, 3, 4)]
    gs += [Geo(3, 100, 1, 20, 64, c) for c in (5, 8, 9, 16)]         # CM = 8, 16
    gs += [Geo(65, 100, 1, 20, 256, 2)]                              # frame_outer loops
    return gs


def _int_cases():
    """(kind, dtype name, variant, Geo) of test (a); variants of one geometry are adjacent
    (they share one cached reference)."""
    cases = []
    for g in _std_geoms():
        only_bf16 = g.N == 512 and g.L == 30                # the CM walk of the N = 512 templates
        cases += [("std", dn, v, g) for dn, v in _variants(g, f32=not only_bf16)]
    cases += [("std", dn, v, Geo(513, 100, 0, 20, 256, 1)) for dn, v in _variants(None, f32=False)]
    cases += [("std", "f32", "valu", Geo(9, 3000, 1, 20, 64, 4))]     # ola_fwd loops
    cases += [("std", "f32", "valu", Geo(2, 100, 1, 20, 512, 16))]    # 72 KB of LDS in dec_fwd
    for g in (Geo(3, 100, 1, 20, 256, 2), Geo(1, 17, 0, 32, 512, 4), Geo(2, 129, 1, 5, 64, 3)):
        cases += [("mask", dn, v, g) for dn, v in _variants(g)]
    return cases


NEVER_RUN = (Geo(3, 100, 1, 32, 512, 2), Geo(2, 100, 1, 20, 512, 16))   # > 64 KB of dynamic LDS in fp32


def _gid(g):
    return f"M{g.M}-K{g.K}{'t' if g.tail else ''}-L{g.L}-N{g.N}-C{g.C}"


def _id(case):
    kind, dn, v, g = case[:4]
    return "-".join([kind, dn, v, _gid(g)] + [str(x) for x in case[4:]])


def _dtype(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _seed(g, salt):
    s = salt
    for v in g:
        s = (s * 4099 + v) % (2 ** 61 - 1)
    return s


def _zero_pad(t, g):
    t.view(g.M, _padded(g.K), -1)[:, g.K:] = 0
    return t


def _tri(shape, gen):
    return torch.randint(-1, 2, shape, generator=gen, dtype=torch.int8).float()


def int_inputs(kind, g):
    """Operands of (a) in {-1, 0, 1} as fp32 on the CPU; the same tensors for the same arguments."""
    gen = torch.Generator().manual_seed(_seed(g, 11 if kind == "std" else 13))
    rows, T = g.M * _padded(g.K), _T(g)
    d = {"V": _tri((g.L, g.N), gen), "w_rows": _zero_pad(_tri((rows, g.N), gen), g), "g_est": _tri((g.M, g.C, T), gen)}
    if kind == "std":
        d["mixture"], d["U"] = _tri((g.M, T), gen), _tri((g.N, g.L), gen)
        d["g_w"] = _zero_pad(_tri((rows, g.N), gen), g)
        d["x_last"] = _zero_pad(_tri((rows, g.C * g.N), gen), g)
        d["Wm"] = None
    else:
        d["x_last"] = _zero_pad(_tri((rows, 8), gen), g)
        col = torch.randint(0, 8, (g.C * g.N,), generator=gen)
        sign = torch.randint(0, 2, (g.C * g.N,), generator=gen).float() * 2 - 1
        d["Wm"] = torch.zeros(g.C * g.N, 8).index_put_((torch.arange(g.C * g.N), col), sign)
    return d


# ----------------------------------------------------------------------------
# fp64 references (CPU), with the optional bf16 rounding model
# ----------------------------------------------------------------------------
class _RoundGrad(torch.autograd.Function):
    """Identity whose gradient is rounded to bf16: a gradient tensor the library stores in bf16."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.bfloat16().double()


def _q(x, on=True):
    """x rounded to bf16 (straight-through for the gradient): a tensor the library stores in bf16."""
    return x + (x.detach().bfloat16().double() - x.detach()) if on else x


def _rg(x, on=True):
    return _RoundGrad.apply(x) if on else x


def _rows(t, g):
    """[M, K, X] -> [M * Kp, X] with zero padded rows."""
    return F.pad(t, (0, 0, 0, _padded(g.K) - g.K)).reshape(g.M * _padded(g.K), -1)


def _valid(t, g):
    return t.double().view(g.M, _padded(g.K), -1)[:, :g.K]


def ref_encoder(g, mixture, U, g_w, bott=None, g_x0=None, model=False):
    """w_rows (and x0) and the parameter gradients of loss = <w_rows, g_w> + <x0, g_x0>."""
    S = _S(g)
    U = U.double().clone().requires_grad_(True)
    x = mixture.double()

    def conv(sig):
        return F.conv1d(sig[:, None], U[:, None], stride=S).transpose(1, 2)   # [M, K, N]

    pre = conv(x)
    assert pre.shape == (g.M, g.K, g.N)
    if model:      # xfr: the mixture frames of the dU column GEMM are bf16; gpre_bf
        pq = conv(_q(x))
        pre = _rg(pq + (pre - pq).detach())
    w32 = torch.relu(pre)
    w = _q(w32, model)
    loss = (w * _valid(g_w, g)).sum()
    out = {"w_rows": _rows(w, g).detach()}
    leaves = [U]
    if bott is not None:
        gamma, beta, Wb = (t.double().clone().requires_grad_(True) for t in bott)
        # the statistics are taken from the fp32 values before w_rows is stored (enc_fwd), and
        # applied to the stored rows
        mean = w32.mean(-1, keepdim=True)
        wh = (w - mean) / torch.sqrt(((w32 - mean) ** 2).mean(-1, keepdim=True) + 1e-8)
        y = _rg(gamma * wh + beta, model)                                      # gcln
        x0 = _q(y @ _q(Wb, model).t(), model)
        loss = loss + (x0 * _valid(g_x0, g)).sum()
        out["x0"] = _rows(x0, g).detach()
        leaves += [gamma, beta, Wb]
    grads = torch.autograd.grad(loss, leaves)
    out.update(zip(("gU", "ggamma0", "gbeta0", "gwb"), grads))
    return out


def _act(score, mask):
    if mask == MASK_SOFTMAX:
        return torch.softmax(score, dim=2)
    return torch.relu(score) if mask == MASK_RELU else score


def _ola(frames, g):
    """frames [M, K, C, L] -> est [M, C, T] (zero from (K - 1) S + L on)."""
    idx = (torch.arange(g.K)[:, None] * _S(g) + torch.arange(g.L)[None, :]).reshape(-1)
    fr = frames.permute(0, 2, 1, 3).reshape(g.M, g.C, g.K * g.L)
    return torch.zeros(g.M, g.C, _T(g), dtype=frames.dtype).index_add(2, idx, fr)


def est_from_score(g, score, w_rows, V, mask):
    """(est, S): the decoder after the mask conv, and the same over absolute values, in fp64."""
    act = _act(_valid(score, g).view(g.M, g.K, g.C, g.N), mask)
    src = _valid(w_rows, g)[:, :, None, :] * act
    return _ola(src @ V.double().t(), g), _ola(src.abs() @ V.double().abs().t(), g)


def ref_decoder(g, x_last, w_rows, Wm, V, g_est, mask, model=False):
    xl = x_last.double().clone().requires_grad_(True)
    wr = w_rows.double().clone().requires_grad_(True)
    Vd = V.double().clone().requires_grad_(True)
    leaves = [xl, wr, Vd]
    x, w = _rg(xl, model), _rg(wr, model)                   # g_x_last and g_w_rows are stored bf16
    if Wm is not None:
        Wd = Wm.double().clone().requires_grad_(True)
        leaves.append(Wd)
        score = _rg(_q(x @ _q(Wd, model).t(), model), model)   # score and gscore
    else:
        score = x
    act = _act(score.view(g.M, _padded(g.K), g.C, g.N)[:, :g.K], mask)
    src = _q(w.view(g.M, _padded(g.K), 1, g.N)[:, :g.K] * act, model)   # srcb
    frames = _rg(src @ Vd.t(), model)                       # gfr
    est = _ola(frames, g)
    grads = torch.autograd.grad(est, leaves, g_est.double())
    out = {"est": est.detach(), "score": score.detach(), "src": src.detach()}
    out.update(zip(("g_x_last", "g_w_rows", "gV", "gwm"), grads))
    return out


@functools.lru_cache(maxsize=1)
def int_reference(kind, g):
    """Inputs, fp64 references and the asserted conditions of one geometry of (a)."""
    d = int_inputs(kind, g)
    mask = MASK_IDENTITY if kind == "std" else MASK_RELU
    ref = {"dec": ref_decoder(g, d["x_last"], d["w_rows"], d["Wm"], d["V"], d["g_est"], mask)}
    operands = [ref["dec"].pop("src"), d["g_est"]]          # src; gfr = frames of dL/dest
    acc = [g.N * 3, g.C * g.L, g.M * g.K * g.C]             # est, g_w, gV
    if kind == "std":
        ref["enc"] = ref_encoder(g, d["mixture"], d["U"], d["g_w"])
        operands += [d["mixture"], d["g_w"]]                # xfr; gpre_bf = g_w under the ReLU mask
        acc += [g.L, g.M * g.K]                             # pre, gU
    else:
        acc += [g.C * g.N * g.L, g.M * g.K * g.L]           # g_x_last, gwm
    cond = {"operand_max": max(float(t.abs().max()) for t in operands),
            "operand_bf16": all(torch.equal(t.float().bfloat16().float(), t.float()) for t in operands),
            "acc_bound": max(acc),
            "ref_max": max(float(v.abs().max()) for r in ref.values() for v in r.values())}
    return d, ref, cond


def _check_conditions(d, cond, g):
    assert cond["operand_max"] <= 256 and cond["operand_bf16"], cond
    assert cond["acc_bound"] < 2 ** 24 and cond["ref_max"] <= cond["acc_bound"], cond
    for k in ("w_rows", "x_last", "g_w"):
        if d.get(k) is not None:
            assert int(d[k].view(g.M, _padded(g.K), -1)[:, g.K:].count_nonzero()) == 0
    for t in d.values():
        if t is not None:
            assert torch.equal(t.bfloat16().float(), t)


# ----------------------------------------------------------------------------
# CPU tests
# ----------------------------------------------------------------------------
def _src(name):
    return open(os.path.join(ROOT, "conv-tasnet_amd", name)).read()


def test_table_constants_match_the_source():
    codec, core, lib = _src("csrc/ctn_codec.hip"), _src("csrc/ctn_capi_core.hip"), _src("ctn_lib.py")

    def num(pat, text=codec):
        return tuple(int(v) for v in re.search(pat, text).groups())

    assert num(r"constexpr int EN_RPB = (\d+);") == (EN_RPB,)
    assert num(r"constexpr int DM_WAVES = (\d+);") == (DM_WAVES,)
    assert num(r"return \(unsigned\)\(wgs < (\d+) \? wgs : (\d+)\);") == (DM_GRID_CAP, DM_GRID_CAP)
    assert num(r"constexpr int FO_R = (\d+), FO_WGS = (\d+), FO_LMAX = (\d+);") == (FO_R, FO_WGS, FO_LMAX)
    assert "return C > 8 ? FO_R / 4 : (C > 4 ? FO_R / 2 : FO_R);" in codec
    assert num(r"if \(gb > (\d+)\) gb = (\d+);\s+hipLaunchKernelGGL\(ola_fwd_kernel") == (OLA_GRID_CAP, OLA_GRID_CAP)
    assert "return dt == BF16 && (a.N == 256 || a.N == 512) && a.L <= 32 && a.C <= 4;" in codec
    assert "dt == BF16 && (!e || atoi(e) != 0) && (a.N == 256 || a.N == 512) && a.L <= 32;" in codec
    assert "blk += (long)gridDim.x * DM_WAVES" in codec and "const long nblk = (long)a.M * Kp / 16;" in codec
    assert num(r"(?m)^ROW_TILE = (\d+)$", lib) == (ROW_TILE,)
    assert num(r"ctn_padded_frames\(int K\) \{ return \(\(K \+ (\d+)\) / (\d+)\) \* (\d+); \}", core) == (
        ROW_TILE - 1, ROW_TILE, ROW_TILE)


def test_geometry_lists_cover_the_edges():
    cases = _int_cases()
    assert len({_id(c) for c in cases}) == len(cases) and len(cases) <= 220
    std = [c for c in cases if c[0] == "std"]
    m1 = {c[3] for c in std if c[3].M == 1 and c[3].N == 256 and c[3].C == 2}
    assert {(g.K, g.tail) for g in m1 if g.L == 20} == {(k, t) for k in KS for t in (0, 1)}
    assert {g.L for g in m1} == set(LS)
    for n in (256, 512):                                    # every CM of both matrix-core templates, run both ways
        for v in ("mfma", "valu"):
            assert {c[3].C for c in std if c[3].N == n and c[1:3] == ("bf16", v)} >= {1, 2, 3, 4}
    for dn in ("bf16", "f32"):                              # CM = 8 and 16 of the VALU kernels
        assert {c[3].C for c in std if c[1] == dn and c[3].N == 64} >= {5, 8, 9, 16}
    assert {c[3].N for c in std} >= {8, 64, 256, 512}
    rows = lambda g: g.M * _padded(g.K)
    assert any(rows(c[3]) > FO_WGS * FO_R and c[2] == "valu" for c in std)            # frame_outer loops
    assert any(rows(c[3]) > DM_GRID_CAP * DM_WAVES * 16 and c[2] == "mfma" for c in std)   # persistent waves loop
    assert any(c[3].M * c[3].C * _T(c[3]) > OLA_GRID_CAP * 256 for c in std)          # ola_fwd loops
    assert any(c[3].L == 32 and c[3].N == 512 and c[1] == "bf16" for c in std)        # Lp == L: no unpad_cols
    for g in NEVER_RUN:
        assert ("std", "f32", "valu", g) in cases
        assert g.N * g.L * 4 + 1 * g.C * g.N * 4 > 64 * 1024                          # dec_fwd at rpb = 1


@pytest.mark.parametrize("kg", sorted({(c[0], c[3]) for c in _int_cases()}), ids=lambda kg: f"{kg[0]}-{_gid(kg[1])}")
def test_int_preconditions_cpu(kg):
    d, _, cond = int_reference(*kg)
    _check_conditions(d, cond, kg[1])


# ----------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------
def _set_variant(monkeypatch, variant, dn):
    for e in ENVS:
        if dn == "f32":
            monkeypatch.delenv(e, raising=False)
        else:
            monkeypatch.setenv(e, "1" if variant == "mfma" else "0")


def _desc(g, B, mask, dt):
    import ctn_ops as ops
    return ops.codec_desc(ops.Frames.of(g.M, g.K), _T(g), g.N, g.L, B, g.C, mask, dt)


def _poison(nbytes):
    """Fill a block of the size the next workspace request will take with NaN bytes and free
    it, so a kernel that skips part of its scratch finds no earlier run's results there."""
    if nbytes:
        torch.empty(int(nbytes), dtype=torch.uint8, device=DEV).fill_(0xFF)


def run_encoder(g, dt, mixture, U, g_w, bott=None, g_x0=None):
    import ctn_lib as L
    import ctn_ops as ops
    fr = ops.Frames.of(g.M, g.K)
    assert fr.Kp == _padded(g.K)
    B = bott[2].shape[0] if bott else 8
    Up = U.to(DEV).view(g.N, 1, g.L).clone().requires_grad_(True)
    ps = [None, None, None]
    if bott:      # the module's parameter shapes: gamma, beta [1, N, 1], bottleneck weight [B, N, 1]
        ps = [t.to(DEV).view(s).clone().requires_grad_(True)
              for t, s in zip(bott, ((1, g.N, 1), (1, g.N, 1), (B, g.N, 1)))]
    d = _desc(g, B, MASK_RELU, dt)
    _poison(L.load().ctn_encoder_workspace_bytes(ctypes.byref(d), 0))
    w_rows, x0 = ops.EncoderFn.apply(mixture.to(DEV), fr, (g.N, g.L, B, 1), dt, Up, *ps)
    outs, cots = [w_rows], [g_w.to(DEV).to(dt)]
    if bott:
        outs.append(x0)
        cots.append(g_x0.to(DEV).to(dt))
    _poison(L.load().ctn_encoder_workspace_bytes(ctypes.byref(d), 1))
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    out = {"w_rows": w_rows.detach().cpu(), "gU": Up.grad.view(g.N, g.L).cpu()}
    if bott:
        out.update(x0=x0.detach().cpu(), ggamma0=ps[0].grad.view(-1).cpu(), gbeta0=ps[1].grad.view(-1).cpu(),
                   gwb=ps[2].grad.view(B, g.N).cpu())
    return out


def run_decoder(g, dt, x_last, w_rows, Wm, V, g_est, mask):
    import ctn_lib as L
    import ctn_ops as ops
    fr = ops.Frames.of(g.M, g.K)
    B = Wm.shape[1] if Wm is not None else 8
    xl = x_last.to(DEV).to(dt).requires_grad_(True)
    wr = w_rows.to(DEV).to(dt).requires_grad_(True)
    Vp = V.to(DEV).clone().requires_grad_(True)
    Wp = Wm.to(DEV).view(g.C * g.N, B, 1).clone().requires_grad_(True) if Wm is not None else None
    d = _desc(g, B, mask, dt)
    _poison(L.load().ctn_decoder_workspace_bytes(ctypes.byref(d), 0))
    est = ops.DecoderFn.apply(xl, wr, fr, (_T(g), g.N, g.L, B, g.C, mask), Wp, Vp)
    score = est.grad_fn.saved_tensors[4] if Wm is not None else None      # what the mask conv stored
    _poison(L.load().ctn_decoder_workspace_bytes(ctypes.byref(d), 1))
    est.backward(g_est.to(DEV))
    torch.cuda.synchronize()
    out = {"est": est.detach().cpu(), "g_x_last": xl.grad.cpu(), "g_w_rows": wr.grad.cpu(), "gV": Vp.grad.cpu()}
    if Wm is not None:
        out.update(gwm=Wp.grad.view(g.C * g.N, B).cpu(), score=score.detach().cpu())
    return out


def _assert_exact(got, ref, what, dt):
    """got == ref (rounded to got's type by torch) everywhere, or a message that names the place."""
    want = ref.to(got.dtype) if got.dtype == torch.float32 else ref.float().to(dt)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    bad |= torch.isnan(got)
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    first = tuple(idx[0].tolist())
    span = ", ".join(f"dim{i} {int(idx[:, i].min())}..{int(idx[:, i].max())}" for i in range(idx.shape[1]))
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong ({span}; on row-layout tensors "
                         f"dim0 / 16 is the matrix-core block); first at {first}: got {float(got[first])}, "
                         f"expected {float(want[first])}")


INT_BF16_OUT = ("w_rows", "g_w_rows", "g_x_last")


def _run_int(kind, g, dt, d):
    out = {}
    if kind == "std":
        out["enc"] = run_encoder(g, dt, d["mixture"], d["U"], d["g_w"])
    out["dec"] = run_decoder(g, dt, d["x_last"], d["w_rows"], d["Wm"], d["V"], d["g_est"],
                             MASK_IDENTITY if kind == "std" else MASK_RELU)
    return out


def _refused_up_front(g, dt):
    """True when codec_check refuses the configuration (0 workspace bytes, CTN_ERR_UNSUPPORTED from
    the forward entry before any launch); raises on any other failure."""
    import ctn_lib as L
    lib = L.load()
    d = _desc(g, 8, MASK_IDENTITY, dt)
    nb = [lib.ctn_encoder_workspace_bytes(ctypes.byref(d), b) for b in (0, 1)]
    nb += [lib.ctn_decoder_workspace_bytes(ctypes.byref(d), b) for b in (0, 1)]
    assert all(n == 0 for n in nb) or all(n > 0 for n in nb), nb
    return nb[0] == 0


@gpu
@pytest.mark.parametrize("case", _int_cases(), ids=_id)
def test_int_exact(case, monkeypatch):
    import ctn_lib as L
    kind, dn, variant, g = case
    dt = _dtype(dn)
    _set_variant(monkeypatch, variant, dn)
    d, ref, cond = int_reference(kind, g)
    _check_conditions(d, cond, g)
    if g in NEVER_RUN and _refused_up_front(g, dt):
        with pytest.raises(L.CtnLibraryError, match=rf"status {ERR_UNSUPPORTED}"):
            _run_int(kind, g, dt, d)
        return
    got = _run_int(kind, g, dt, d)
    for part, r in ref.items():
        for name, want in r.items():
            if name in got[part]:
                o = got[part][name]
                assert o.dtype == (dt if name in INT_BF16_OUT or name == "score" else torch.float32), (name, o.dtype)
                _assert_exact(o, want, f"{part}.{name}", dt)
    assert set(got["dec"]) - {"score"} <= set(ref["dec"]) and ("enc" not in got or set(got["enc"]) <= set(ref["enc"]))
    again = _run_int(kind, g, dt, d)
    for part in got:
        for name in got[part]:
            assert torch.equal(got[part][name], again[part][name]), f"run to run: {part}.{name}"


# ---- (c) real-valued arithmetic ---------------------------------------------
EGeo = collections.namedtuple("EGeo", "M K tail L N B")
ENC_GAUSS = (EGeo(3, 100, 1, 20, 256, 128), EGeo(1, 17, 0, 16, 512, 64), EGeo(2, 129, 1, 30, 64, 40),
             EGeo(2, 97, 1, 32, 256, 128), EGeo(3, 100, 0, 5, 8, 8))
DGeo = collections.namedtuple("DGeo", "M K tail L N C B")
DEC_GAUSS = (DGeo(3, 100, 1, 20, 256, 2, 128), DGeo(1, 17, 0, 16, 512, 3, 64), DGeo(2, 129, 1, 30, 256, 4, 40),
             DGeo(2, 97, 1, 32, 512, 1, 128), DGeo(3, 100, 0, 5, 64, 5, 8))
MASKS = {"relu": MASK_RELU, "softmax": MASK_SOFTMAX, "identity": MASK_IDENTITY}
EPS_ACT = {"relu": 0.0, "identity": 0.0, "softmax": 2.0 ** -16}    # softmax: an assumption (docstring)


def _store(t, dt):
    return t.to(dt).float()


@functools.lru_cache(maxsize=1)
def enc_gauss_reference(eg, dn):
    dt = _dtype(dn)
    g = Geo(eg.M, eg.K, eg.tail, eg.L, eg.N, 1)
    gen = torch.Generator().manual_seed(_seed(eg, 17))
    rows, T = g.M * _padded(g.K), _T(g)
    d = {"mixture": torch.randn(g.M, T, generator=gen), "U": torch.randn(g.N, g.L, generator=gen) / g.L ** 0.5,
         "gamma": 1 + 0.1 * torch.randn(g.N, generator=gen), "beta": 0.1 * torch.randn(g.N, generator=gen),
         "Wb": torch.randn(eg.B, g.N, generator=gen) / g.N ** 0.5,
         "g_w": _store(_zero_pad(torch.randn(rows, g.N, generator=gen), g), dt),
         "g_x0": _store(_zero_pad(torch.randn(rows, eg.B, generator=gen), g), dt)}
    bott = (d["gamma"], d["beta"], d["Wb"])
    ref = ref_encoder(g, d["mixture"], d["U"], d["g_w"], bott, d["g_x0"])
    model = ref_encoder(g, d["mixture"], d["U"], d["g_w"], bott, d["g_x0"], model=True) if dn == "bf16" else ref
    xf = d["mixture"].double().unfold(-1, g.L, _S(g))[:, :g.K]
    S_w = _rows(xf.abs() @ d["U"].double().abs().t(), g)
    return g, d, ref, model, S_w


@functools.lru_cache(maxsize=1)
def dec_gauss_reference(dg, dn, mname):
    dt = _dtype(dn)
    g = Geo(dg.M, dg.K, dg.tail, dg.L, dg.N, dg.C)
    gen = torch.Generator().manual_seed(_seed(dg, 19 + MASKS[mname]))
    rows, T = g.M * _padded(g.K), _T(g)
    ident = mname == "identity"
    cin = g.C * g.N if ident else dg.B
    d = {"x_last": _store(_zero_pad(torch.randn(rows, cin, generator=gen).clamp_(-8, 8), g), dt),
         "Wm": None if ident else torch.randn(g.C * g.N, dg.B, generator=gen) / dg.B ** 0.5,
         "w_rows": _store(_zero_pad(torch.randn(rows, g.N, generator=gen).abs_(), g), dt),
         "V": torch.randn(g.L, g.N, generator=gen) / g.N ** 0.5, "g_est": torch.randn(g.M, g.C, T, generator=gen)}
    args = (g, d["x_last"], d["w_rows"], d["Wm"], d["V"], d["g_est"], MASKS[mname])
    ref = ref_decoder(*args)
    model = ref_decoder(*args, model=True) if dn == "bf16" else ref
    return g, d, ref, model


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _elementwise(got, ref, bound, what):
    assert bool(torch.isfinite(got).all()), what
    err = (got.double() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    return ratio, bool((err <= bound).all())          # 0 <= 0 on padded rows and the tail


def _composite(got, ref, model, names, label):
    fails = []
    for n in names:
        e_k, e_m = _rel(got[n], ref[n]), _rel(model[n], ref[n])
        print(f"  {label} {n}: rel L2 kernel {e_k:.3e}, rounding model {e_m:.3e}, bound {2 * e_m + 1e-5:.3e}")
        assert bool(torch.isfinite(got[n]).all()), n
        if not e_k <= 2 * e_m + 1e-5:
            fails.append((n, e_k, e_m))
    return fails


def _gauss_variants():
    return [("bf16", "mfma"), ("bf16", "valu"), ("f32", "valu")]


@gpu
@pytest.mark.parametrize("case", [("enc", dn, v, eg) for eg in ENC_GAUSS for dn, v in _gauss_variants()],
                         ids=lambda c: f"{c[1]}-{c[2]}-" + "-".join(f"{k}{x}" for k, x in zip(EGeo._fields, c[3])))
def test_gauss_elementwise_encoder(case, monkeypatch):
    """Encoder front with the bottleneck: w_rows per element; x0, gU, ggamma0, gbeta0, gwb against
    the rounding model."""
    _, dn, variant, eg = case
    dt = _dtype(dn)
    _set_variant(monkeypatch, variant, dn)
    g, d, ref, model, S_w = enc_gauss_reference(eg, dn)
    got = run_encoder(g, dt, d["mixture"], d["U"], d["g_w"], (d["gamma"], d["beta"], d["Wb"]), d["g_x0"])
    u = 2.0 ** -8 if dn == "bf16" else 0.0
    ratio, ok = _elementwise(got["w_rows"], ref["w_rows"], u * ref["w_rows"].abs() + g.L * 2.0 ** -23 * S_w, "w_rows")
    print(f"\ncodec {_id(case[:3] + (g,))}: w_rows worst error/bound {ratio:.3f}")
    fails = _composite(got, ref, model, ("x0", "gU", "ggamma0", "gbeta0", "gwb"), "enc")
    assert ok, f"w_rows: worst error/bound {ratio}"
    assert not fails, fails
    for n in ("w_rows", "x0"):
        assert int(got[n].view(g.M, _padded(g.K), -1)[:, g.K:].count_nonzero()) == 0, n


@gpu
@pytest.mark.parametrize("case", [("dec", dn, v, dg, m) for dg in DEC_GAUSS for m in MASKS for dn, v in _gauss_variants()],
                         ids=lambda c: f"{c[4]}-{c[1]}-{c[2]}-" + "-".join(f"{k}{x}" for k, x in zip(DGeo._fields, c[3])))
def test_gauss_elementwise_decoder(case, monkeypatch):
    """Decoder back with the mask conv and relu / softmax (and the standalone identity form): score
    and est per element; g_x_last, g_w_rows, gwm, gV against the rounding model."""
    _, dn, variant, dg, mname = case
    dt = _dtype(dn)
    _set_variant(monkeypatch, variant, dn)
    g, d, ref, model = dec_gauss_reference(dg, dn, mname)
    mask = MASKS[mname]
    got = run_decoder(g, dt, d["x_last"], d["w_rows"], d["Wm"], d["V"], d["g_est"], mask)
    u = 2.0 ** -8 if dn == "bf16" else 0.0
    label = f"{mname}-{dn}-{variant}-{_gid(g)}"
    if d["Wm"] is not None:
        wm = _store(d["Wm"], dt).double()                    # the operand the GEMM sees: the bf16 weight copy
        sref = d["x_last"].double() @ wm.t()
        sabs = d["x_last"].double().abs() @ wm.abs().t()
        rs, oks = _elementwise(got["score"], sref, u * sref.abs() + dg.B * 2.0 ** -23 * sabs, "score")
        assert float(got["score"].abs().max()) <= 8, "precondition |score| <= 8"
        assert int(got["score"].view(g.M, _padded(g.K), -1)[:, g.K:].count_nonzero()) == 0
        score = got["score"]
    else:
        rs, oks, score = 0.0, True, d["x_last"]
    eref, S = est_from_score(g, score, d["w_rows"], d["V"], mask)
    re_, oke = _elementwise(got["est"], eref, (2 * u + g.N * 2.0 ** -23 + EPS_ACT[mname]) * S, "est")
    print(f"\ncodec dec {label}: worst error/bound score {rs:.3f} est {re_:.3f}")
    names = ("g_x_last", "g_w_rows", "gV") + (("gwm",) if d["Wm"] is not None else ())
    fails = _composite(got, ref, model, names, "dec")
    assert oks, f"score: worst error/bound {rs}"
    assert oke, f"est: worst error/bound {re_}"
    assert not fails, fails
    last = (g.K - 1) * _S(g) + g.L
    assert int(got["est"][:, :, last:].count_nonzero()) == 0
    for n in ("g_x_last", "g_w_rows"):
        assert int(got[n].view(g.M, _padded(g.K), -1)[:, g.K:].count_nonzero()) == 0, n


# ---- (d) guard bands, padding and tails --------------------------------------
GUARD = 4096        # bytes of 0xA5 on either side
BAND = 0xA5


class _Guarded:
    """A tensor of `shape` between two sentinel bands inside one larger byte buffer."""

    def __init__(self, shape, dtype, fill=float("nan")):
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((2 * GUARD + self.nbytes,), BAND, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        if dtype == torch.uint8:
            self.t.fill_(0xFF)
        else:
            self.t.fill_(fill)

    def intact(self):
        return bool((self.raw[:GUARD] == BAND).all()) and bool((self.raw[GUARD + self.nbytes:] == BAND).all())


GUARD_CASES = [  # dtype name, variant, Geo, B, mask
    ("bf16", "mfma", Geo(3, 97, 1, 20, 256, 2), 64, "relu"), ("bf16", "valu", Geo(3, 97, 1, 20, 256, 2), 64, "relu"),
    ("f32", "valu", Geo(3, 97, 1, 20, 256, 2), 64, "softmax"), ("bf16", "mfma", Geo(2, 17, 1, 30, 512, 3), 40, "softmax"),
    ("bf16", "mfma", Geo(2, 129, 1, 32, 256, 4), 8, "identity"), ("bf16", "valu", Geo(1, 1, 1, 16, 64, 5), 8, "identity"),
    ("f32", "valu", Geo(2, 100, 1, 5, 8, 9), 16, "relu"), ("bf16", "mfma", Geo(5, 127, 1, 20, 512, 1), 128, "relu"),
]


def _guard_pipeline(lib, g, dt, B, mask, d, tail_value):
    """Encoder front and decoder back, forward and backward, through the C ABI with guarded outputs
    and workspaces; the mixture and dL/dest samples past (K - 1) S + L hold tail_value."""
    import ctn_lib as L
    rows, T, last = g.M * _padded(g.K), _T(g), (g.K - 1) * _S(g) + g.L
    assert last < T
    dev = lambda t: t.to(DEV).contiguous()
    mix, g_est = d["mixture"].clone(), d["g_est"].clone()
    mix[:, last:] = tail_value
    g_est[:, :, last:] = tail_value
    mix, g_est, U, gamma, beta, Wb, V = (dev(t) for t in (mix, g_est, d["U"], d["gamma"], d["beta"], d["Wb"], d["V"]))
    g_w, g_x0, x_last = (dev(d[k].to(dt)) for k in ("g_w", "g_x0", "x_last"))
    Wm = dev(d["Wm"]) if d["Wm"] is not None else None
    stream = L.stream_handle(torch.device(DEV))
    out, guards = {}, []

    def G(name, shape, dtype):
        o = _Guarded(shape, dtype)
        guards.append((name, o))
        if name != "ws":
            out[name] = o.t
        return o.t

    def ws(fn, backward):
        nb = fn(ctypes.byref(desc), backward)
        assert nb > 0
        return G("ws", (nb,), torch.uint8), nb

    desc = _desc(g, B, MASK_RELU, dt)
    w_rows, stats, x0 = G("w_rows", (rows, g.N), dt), G("cln_stats", (rows, 2), torch.float32), G("x0", (rows, B), dt)
    w, nb = ws(lib.ctn_encoder_workspace_bytes, 0)
    L.check(lib.ctn_encoder_forward(ctypes.byref(desc), mix.data_ptr(), U.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                    Wb.data_ptr(), w_rows.data_ptr(), stats.data_ptr(), x0.data_ptr(), w.data_ptr(), nb,
                                    stream), "ctn_encoder_forward")
    gU, gg0, gb0 = G("gU", (g.N, g.L), torch.float32), G("ggamma0", (g.N,), torch.float32), G("gbeta0", (g.N,), torch.float32)
    gwb = G("gwb", (B, g.N), torch.float32)
    w, nb = ws(lib.ctn_encoder_workspace_bytes, 1)
    L.check(lib.ctn_encoder_backward(ctypes.byref(desc), mix.data_ptr(), U.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                     Wb.data_ptr(), w_rows.data_ptr(), stats.data_ptr(), g_w.data_ptr(), g_x0.data_ptr(),
                                     gU.data_ptr(), gg0.data_ptr(), gb0.data_ptr(), gwb.data_ptr(), w.data_ptr(), nb,
                                     stream), "ctn_encoder_backward")
    desc = _desc(g, B, mask, dt)
    cin = B if Wm is not None else g.C * g.N
    score = G("score", (rows, g.C * g.N), dt) if Wm is not None else None
    est = G("est", (g.M, g.C, T), torch.float32)
    w, nb = ws(lib.ctn_decoder_workspace_bytes, 0)
    L.check(lib.ctn_decoder_forward(ctypes.byref(desc), x_last.data_ptr(), w_rows.data_ptr(), L.ptr(Wm), V.data_ptr(),
                                    L.ptr(score), est.data_ptr(), w.data_ptr(), nb, stream), "ctn_decoder_forward")
    g_x, g_wr = G("g_x_last", (rows, cin), dt), G("g_w_rows", (rows, g.N), dt)
    gwm = G("gwm", (g.C * g.N, B), torch.float32) if Wm is not None else None
    gV = G("gV", (g.L, g.N), torch.float32)
    w, nb = ws(lib.ctn_decoder_workspace_bytes, 1)
    L.check(lib.ctn_decoder_backward(ctypes.byref(desc), x_last.data_ptr(), w_rows.data_ptr(), L.ptr(Wm), V.data_ptr(),
                                     L.ptr(score), g_est.data_ptr(), g_x.data_ptr(), g_wr.data_ptr(), L.ptr(gwm),
                                     gV.data_ptr(), w.data_ptr(), nb, stream), "ctn_decoder_backward")
    torch.cuda.synchronize()
    for name, o in guards:
        assert o.intact(), f"{name}: sentinel band overwritten"
    return {k: v.clone() for k, v in out.items()}


@gpu
@pytest.mark.parametrize("case", GUARD_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{_gid(c[2])}-B{c[3]}-{c[4]}")
def test_guard_bands_and_padding(case, monkeypatch):
    import ctn_lib as L
    dn, variant, g, B, mname = case
    dt = _dtype(dn)
    _set_variant(monkeypatch, variant, dn)
    lib = L.load()
    gen = torch.Generator().manual_seed(_seed(g, 23 + B))
    rows, T = g.M * _padded(g.K), _T(g)
    ident = mname == "identity"
    d = {"mixture": torch.randn(g.M, T, generator=gen), "U": torch.randn(g.N, g.L, generator=gen) / g.L ** 0.5,
         "gamma": 1 + 0.1 * torch.randn(g.N, generator=gen), "beta": 0.1 * torch.randn(g.N, generator=gen),
         "Wb": torch.randn(B, g.N, generator=gen) / g.N ** 0.5,
         "g_w": _zero_pad(torch.randn(rows, g.N, generator=gen), g),
         "g_x0": _zero_pad(torch.randn(rows, B, generator=gen), g),
         "x_last": _zero_pad(torch.randn(rows, g.C * g.N if ident else B, generator=gen), g),
         "Wm": None if ident else torch.randn(g.C * g.N, B, generator=gen) / B ** 0.5,
         "V": torch.randn(g.L, g.N, generator=gen) / g.N ** 0.5, "g_est": torch.randn(g.M, g.C, T, generator=gen)}
    a = _guard_pipeline(lib, g, dt, B, MASKS[mname], d, 1000.0)
    for name, t in a.items():
        assert not bool(torch.isnan(t).any()), f"{name}: NaN left (rows never written)"
    pad = lambda t: t.view(g.M, _padded(g.K), -1)[:, g.K:]
    for name in ("w_rows", "x0", "g_w_rows", "g_x_last") + (() if ident else ("score",)):
        assert int(pad(a[name]).count_nonzero()) == 0, f"{name}: padded rows not zero"
    st = pad(a["cln_stats"])
    assert bool((st[..., 0] == 0).all()) and bool((st[..., 1] == 1).all()), "cLN statistics of padded rows != (0, 1)"
    last = (g.K - 1) * _S(g) + g.L
    assert int(a["est"][:, :, last:].count_nonzero()) == 0 and int(a["est"][:, :, :last].count_nonzero()) > 0
    b = _guard_pipeline(lib, g, dt, B, MASKS[mname], d, -777.0)
    for name in a:
        assert torch.equal(a[name].view(torch.uint8), b[name].view(torch.uint8)), f"{name}: depends on tail samples"
