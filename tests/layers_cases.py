"""Cases, inputs, oracle and comparator shared by test_layers_oracle.py (CPU) and
test_gpu_layers_alone.py (GPU); no tests here.

A case is a tuple that starts with its op:

    ("gLN" | "cLN", M, K, C)          layer norms, conv_tasnet.py:307-355
    ("prelu", M, K, C, alpha)         nn.PReLU(), one shared alpha
    ("dw", M, K, C, P, dil, causal)   conv1d(groups=C) with the reference's padding (+ Chomp1d)
    ("relu" | "softmax", M, K, N, S)  mask nonlinearity over S speakers, channel s*N + n

Every tensor of a case lives in the frame-row layout [M, Kp, C], padded
rows included, and the oracle takes exactly what the kernels take: it cuts the K valid rows
out itself, evaluates plain torch in the dtype it is given (float64 is the reference,
float32 the yardstick of test_layers_oracle.py), pads the result with zero rows and lets
autograd produce the gradients.  What sits in the padded rows of x and gy can therefore not
reach anything the oracle returns, which is the contract the poisoned-padding cases hold the
kernels to.

`wrong=` selects a named wrong variant of the oracle (WRONG below): what a kernel with one
specific defect would compute.  test_layers_oracle.py shows that the comparator rejects each
at the case meant to catch it.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-8        # conv_tasnet.py:10
ROW_TILE = 128    # Kp = ceil(K / 128) * 128
LY_RB = 64        # rows per partial block of ctn_layers.hip
KINK = 3e-6       # x rms: nearest an input may come to PReLU's / relu's kink unless it is exactly 0
POISON = 1e4

NORMS = ("gLN", "cLN")
MASKS = ("relu", "softmax")


def padded(K):
    return -(-K // ROW_TILE) * ROW_TILE


def case_id(c):
    return "-".join(str(v) for v in c)


# ----------------------------------------------------------------------------
# the case tables
# ----------------------------------------------------------------------------
# nparts of slab_reduce = M * Kp / 64: 2, 30, 32, 34, 66 at K = 100
PARTS_TABLE = [(M, 100) for M in (1, 15, 16, 17, 33)]
BIG = (9, 1000, 128)      # 1.18 M elements: past ew_grid's 4096 x 256 threads

LN_GEOMETRY = (
    [(2, K, 24) for K in (1, 63, 64, 65, 128, 129, 448, 449, 513)]   # nb = 1 1 1 2 2 3 7 8 9
    + [(65, 65, 8), (257, 10, 8)]                                   # two tiles / two thread workgroups
    + [(M, K, 24) for M, K in PARTS_TABLE]
    + [(3, 300, C) for C in (1, 6, 7, 24, 64, 65, 130)]
    + [BIG]
)
LN_CASES = [(n,) + g for n in NORMS for g in LN_GEOMETRY]

ALPHAS = (-0.5, 0.0, 0.25, 1.5)
PRELU_CASES = (
    [("prelu", 3, 300, C, a) for C in (24, 7) for a in ALPHAS]
    + [("prelu", M, K, 24, 0.25) for M, K in PARTS_TABLE]
    + [("prelu",) + BIG + (0.25,)]
)

DW_GEO = [(3, 1, 0), (3, 1, 1), (3, 4, 0), (3, 128, 0), (3, 128, 1), (1, 1, 0), (2, 1, 1), (2, 3, 1), (5, 2, 0)]
DW_CASES = (
    [("dw", M, K, C) + g for M, K in ((3, 300), (2, 128)) for C in (7, 8, 64) for g in DW_GEO]
    + [("dw", 2, 100, 8, 3, 128, c) for c in (0, 1)]           # every tap but one outside
    + [("dw", 2, 129, 8, 3, 1, 1)]                              # the poisoned / bf16 geometry
)
DW_UNSUPPORTED = [(2, 1), (2, 3), (4, 1)]                       # non-causal, (P - 1) * dil odd

MASK_CASES = (
    [(t, 3, 300, N, S) for t in MASKS for N in (24, 64) for S in (1, 2, 3, 5)]
    + [(t, 2, 129, 24, 2) for t in MASKS]
)

FP32_CASES = LN_CASES + PRELU_CASES + DW_CASES + MASK_CASES

POISON_CASES = (
    [(n, M, K, 24) for n in NORMS for M, K in ((3, 300), (2, 129))]
    + [("dw", 3, 300, 8, 3, 4, 0), ("dw", 2, 129, 8, 3, 1, 1)]
    + [("softmax", 3, 300, 24, 3), ("relu", 3, 300, 24, 3), ("softmax", 2, 129, 24, 2), ("relu", 2, 129, 24, 2)]
)
BF16_CASES = POISON_CASES + [("prelu", 3, 300, 24, 0.25), ("prelu", 2, 129, 24, 0.25)]
DETERMINISM_CASES = [("gLN", 17, 100, 24), ("cLN", 17, 100, 24), ("prelu", 17, 100, 24, 0.25),
                     ("dw", 3, 300, 7, 3, 4, 0), ("softmax", 3, 300, 24, 3)]

# wrong variant -> (the case meant to catch it, poisoned padding, the tensors it must break)
WRONG = {
    "gln_count_kp": (("gLN", 2, 65, 24), False, ("y", "gx", "stats")),
    "gln_drop_last_block": (("gLN", 2, 65, 24), False, ("y", "gx", "stats")),
    "ggrads_drop_parts_32": (("gLN", 17, 100, 24), False, ("ggamma", "gbeta")),
    "ggrads_drop_parts_32_cln": (("cLN", 17, 100, 24), False, ("ggamma", "gbeta")),
    "ggrads_padded_rows": (("gLN", 3, 300, 24), True, ("ggamma", "gbeta")),
    "ggrads_padded_rows_cln": (("cLN", 2, 129, 24), True, ("ggamma", "gbeta")),
    "dw_cross_utterance": (("dw", 2, 128, 8, 3, 1, 0), False, ("y", "gx", "gw")),
    "dw_cross_utterance_causal": (("dw", 2, 128, 8, 3, 128, 1), False, ("y", "gx", "gw")),
    "softmax_no_max": (("softmax", 3, 300, 24, 3), False, ("y", "gx")),
    "prelu_slope_1_at_0": (("prelu", 3, 300, 24, 0.25), False, ("gx",)),
}


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _seed(case):
    s = 12345
    for v in case:
        v = {"gLN": 1, "cLN": 2, "prelu": 3, "dw": 4, "relu": 5, "softmax": 6}.get(v, v)
        s = (s * 1000003 + int(round(float(v) * 64)) + 7) % (2 ** 31 - 1)
    return s


def channels(case):
    return case[3] * case[4] if case[0] in MASKS else case[3]


@functools.lru_cache(maxsize=None)
def make_inputs(case, bf16=False, poison=False):
    """-> dict of fp32 tensors: x and gy as rows [M, Kp, C] (padded rows zero, or +-1e4 with
    poison: the valid rows are the same numbers either way), and the op's parameters.  With
    bf16, x and gy are rounded to bf16 first, so the oracle sees what the kernels read;
    parameters stay fp32 as in the library."""
    op, M, K = case[:3]
    C, Kp = channels(case), padded(K)
    g = torch.Generator().manual_seed(_seed(case))

    def rn(*s):
        return torch.randn(*s, generator=g)

    def ru(*s):
        return torch.rand(*s, generator=g)

    inp = {}
    if op in NORMS:
        # every channel sits 1.5 to 2.5 standard deviations of the noise away from zero, all on
        # one side, so each group's E[x^2] - mean^2 is a real subtraction (|mean| / std ~ 1.9)
        sign = 1.0 if _seed(case) % 2 else -1.0
        x = rn(M, K, C) + 2.0 * sign * (1.0 + 0.25 * (2 * ru(1, 1, C) - 1))
        inp["gamma"] = 1.0 + 0.3 * (2 * ru(1, C, 1) - 1)
        inp["beta"] = 0.3 * (2 * ru(1, C, 1) - 1)
    elif op == "prelu":
        x = 1.5 * rn(M, K, C)
        x[ru(M, K, C) < 0.05] = 0.0          # exactly on the kink: slope alpha there
        inp["alpha"] = torch.tensor([float(case[4])])
    elif op == "dw":
        P = case[4]
        x = 1.5 * rn(M, K, C)
        inp["w"] = rn(C, 1, P) / P ** 0.5
    else:
        N, S = case[3], case[4]
        s = 3.0 * rn(M, K, S, N)
        alt = torch.tensor([1.0 if i % 2 == 0 else -1.0 for i in range(S)]).view(1, 1, S, 1)
        k = torch.arange(K) % 10
        s[:, k == 0] = 80.0                  # every speaker at +80
        s[:, k == 1] = -80.0
        s[:, k == 2] = (80.0 * alt).expand(M, int((k == 2).sum()), S, N)
        # exp(80) = 5.5e34 still fits fp32 (exp overflows past 88.7), so +-80 alone would let a
        # softmax without the max subtraction through; +-100 does overflow (and exp(-100) is
        # denormal), which is what the wrong variant softmax_no_max is caught by
        s[:, k == 3] = (100.0 * alt).expand(M, int((k == 3).sum()), S, N)
        s[:, k == 4] = -100.0
        if S > 1:
            s[:, k == 5, 1] = s[:, k == 5, 0]   # exact tie between two speakers
        s[:, k == 6, 0] = 0.0                # relu input exactly 0
        x = s.reshape(M, K, C)
    if op == "prelu" or op in MASKS:
        # nothing but the exact zeros within KINK x rms of the kink (rms is 1.5 for PReLU and
        # below 100 for the masks, so the band is narrower than 3e-4)
        near = (x != 0) & (x.abs() < 1e-3)
        x[near] = 1e-3 * torch.sign(x[near])
    gy = rn(M, K, C)
    if bf16:
        x, gy = x.bfloat16().float(), gy.bfloat16().float()
    xr, gyr = torch.zeros(M, Kp, C), torch.zeros(M, Kp, C)
    xr[:, :K], gyr[:, :K] = x, gy
    if poison and Kp > K:
        gp = torch.Generator().manual_seed(_seed(case) + 1)
        for t in (xr, gyr):
            t[:, K:] = POISON * (2.0 * torch.randint(0, 2, (M, Kp - K, C), generator=gp) - 1.0)
    inp["x"], inp["gy"] = xr, gyr
    return inp


# ----------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------
def _leaf(t, dtype):
    """A fresh leaf in `dtype`: the cached inputs are shared and stay untouched."""
    return t.detach().to(dtype, copy=True).requires_grad_(True)


def _rows(t_ncw, Kp):
    """[M, C, K] -> rows [M, Kp, C], padded rows zero."""
    return F.pad(t_ncw.transpose(1, 2), (0, 0, 0, Kp - t_ncw.shape[2]))


def _ln(case, inp, dtype, wrong):
    norm, M, K, C = case
    Kp = padded(K)
    xr = _leaf(inp["x"], dtype)
    gamma = _leaf(inp["gamma"], dtype)
    beta = _leaf(inp["beta"], dtype)
    gyr = inp["gy"].to(dtype)
    x = xr[:, :K].transpose(1, 2)                                   # [M, C, K]
    if norm == "cLN":                                               # conv_tasnet.py:319-329
        mean = torch.mean(x, dim=1, keepdim=True)
        var = torch.var(x, dim=1, keepdim=True, unbiased=False)
    else:                                                           # conv_tasnet.py:344-355
        mean = x.mean(dim=1, keepdim=True).mean(dim=2, keepdim=True)
        var = (torch.pow(x - mean, 2)).mean(dim=1, keepdim=True).mean(dim=2, keepdim=True)
    if wrong in ("gln_count_kp", "gln_drop_last_block"):
        assert norm == "gLN"
        if wrong == "gln_count_kp":      # the statistics divided by the padded row count
            xs, cnt = x, Kp * C
        else:                            # the last row block's partial never added
            xs, cnt = x[:, :, :(-(-K // LY_RB) - 1) * LY_RB], K * C
        mean = xs.sum((1, 2), keepdim=True) / cnt
        var = (xs * xs).sum((1, 2), keepdim=True) / cnt - mean * mean
    y = gamma * (x - mean) / torch.pow(var + EPS, 0.5) + beta
    yr = _rows(y, Kp)
    yr.backward(gyr)
    with torch.no_grad():
        rstd = 1.0 / torch.sqrt(var + EPS)
        if norm == "gLN":
            stats = torch.stack([mean.reshape(M), rstd.reshape(M)], 1)               # [M, 2]
        else:
            stats = torch.stack([mean.reshape(M, K), rstd.reshape(M, K)], 2)         # [M, K, 2]
        out = {"y": yr.detach(), "gx": xr.grad, "ggamma": gamma.grad, "gbeta": beta.grad, "stats": stats}
        if wrong and wrong.startswith("ggrads"):
            g = gyr[:, :K].transpose(1, 2)
            xhat = (x - mean) * rstd
            keep = torch.ones(M, 1, K, dtype=dtype)
            if "drop_parts_32" in wrong:  # row blocks 32.. of the [M * Kp] rows never summed
                flat = (torch.arange(M).view(M, 1, 1) * Kp + torch.arange(K).view(1, 1, K))
                keep = (flat < 32 * LY_RB).to(dtype)
            gg, gb = (g * xhat * keep).sum((0, 2)), (g * keep).sum((0, 2))
            if "padded_rows" in wrong:    # padded rows summed like valid ones
                xp, gp = xr[:, K:].detach(), gyr[:, K:]                               # [M, Kp-K, C]
                if norm == "gLN":
                    xhp = (xp - mean.reshape(M, 1, 1)) * rstd.reshape(M, 1, 1)
                else:
                    xhp = (xp - xp.mean(2, keepdim=True)) / torch.sqrt(xp.var(2, keepdim=True, unbiased=False) + EPS)
                gg, gb = gg + (gp * xhp).sum((0, 1)), gb + gp.sum((0, 1))
            out["ggamma"], out["gbeta"] = gg.view(1, C, 1), gb.view(1, C, 1)
        ratio = float((mean.abs() / var.sqrt().clamp_min(1e-300)).median())
    return out, {"mean_over_std": ratio}


def _kink(v):
    """Least |v| / rms(v) over the elements of v that are not exactly 0."""
    nz = v[v != 0]
    return float(nz.abs().min() / v.square().mean().sqrt())


def _prelu(case, inp, dtype, wrong):
    _, M, K, C, _ = case
    # PReLU's contract is zero padded rows on input: prelu(0) = 0 keeps y's padded rows
    # zero, a zero gy there keeps gx's, and 0 adds nothing to the alpha gradient.  The
    # kernels do not test k < K, so neither does this restatement.
    xr = _leaf(inp["x"], dtype)
    alpha = _leaf(inp["alpha"], dtype)
    gyr = inp["gy"].to(dtype)
    assert not xr[:, K:].any() and not gyr[:, K:].any()
    y = F.prelu(xr, alpha)
    y.backward(gyr)
    out = {"y": y.detach(), "gx": xr.grad, "galpha": alpha.grad}
    if wrong == "prelu_slope_1_at_0":
        out["gx"] = gyr * torch.where(xr.detach() >= 0, torch.ones_like(gyr), alpha.detach().expand_as(gyr))
    return out, {"kink": _kink(xr.detach()[:, :K]), "zeros": int((xr[:, :K] == 0).sum())}


def _dw(case, inp, dtype, wrong):
    _, M, K, C, P, dil, causal = case
    Kp = padded(K)
    xr = _leaf(inp["x"], dtype)
    w = _leaf(inp["w"], dtype)
    gyr = inp["gy"].to(dtype)
    pad = (P - 1) * dil

    def conv(x):   # conv_tasnet.py:188, 262-265, 275-289
        if causal:
            return F.conv1d(x, w, padding=pad, dilation=dil, groups=C)[:, :, :x.shape[2]]   # Chomp1d(pad)
        assert pad % 2 == 0
        return F.conv1d(x, w, padding=pad // 2, dilation=dil, groups=C)

    if wrong and wrong.startswith("dw_cross_utterance"):
        # taps bounded by the whole buffer instead of the utterance: one long signal
        flat = xr.reshape(1, M * Kp, C).transpose(1, 2)
        yr = conv(flat).transpose(1, 2).reshape(M, Kp, C)
        yr = yr * (torch.arange(Kp) < K).to(dtype).view(1, Kp, 1)
    else:
        yr = _rows(conv(xr[:, :K].transpose(1, 2)), Kp)
    yr.backward(gyr * (torch.arange(Kp) < K).to(dtype).view(1, Kp, 1))
    return {"y": yr.detach(), "gx": xr.grad, "gw": w.grad}, {}


def _mask(case, inp, dtype, wrong):
    kind, M, K, N, S = case
    Kp = padded(K)
    xr = _leaf(inp["x"], dtype)
    gyr = inp["gy"].to(dtype)
    s = xr[:, :K].reshape(M, K, S, N)
    if kind == "relu":                       # conv_tasnet.py:202-208
        m = F.relu(s)
    elif wrong == "softmax_no_max":
        e = torch.exp(s)
        m = e / e.sum(2, keepdim=True)
    else:
        m = F.softmax(s, dim=2)
    yr = F.pad(m.reshape(M, K, S * N), (0, 0, 0, Kp - K))
    yr.backward(gyr)
    return {"y": yr.detach(), "gx": xr.grad}, {"kink": _kink(s.detach())}


def oracle(case, inp, dtype=torch.float64, wrong=None):
    """One forward + backward of the case in `dtype` on the CPU -> ({name: tensor}, conditioning).
    y and gx are rows [M, Kp, C] with zero padded rows; parameter gradients have the
    parameters' shapes; stats is [M, 2] (gLN) or [M, K, 2] (cLN, valid rows): (mean, rstd)."""
    op = case[0]
    fn = _ln if op in NORMS else _prelu if op == "prelu" else _dw if op == "dw" else _mask
    return fn(case, inp, dtype, wrong)


@functools.lru_cache(maxsize=None)
def reference(case, bf16=False, poison=False):
    return oracle(case, make_inputs(case, bf16, poison))


def check_conditioning(case, cond):
    """The fp32 cases are well conditioned where they claim to be."""
    if case[0] in NORMS:
        assert cond["mean_over_std"] >= 1.0, cond
    elif case[0] == "prelu":
        assert cond["kink"] >= KINK and cond["zeros"] > 0, cond
    elif case[0] == "relu":
        assert cond["kink"] >= KINK, cond


# ----------------------------------------------------------------------------
# the comparator
# ----------------------------------------------------------------------------
# the project's fp32 numbers per element (test_gpu_bn_block.py holds the same arithmetic to them)
FP32 = {"y": (1e-4, 1e-4), "gx": (1e-4, 2e-4), "stats": (1e-4, 1e-5)}


def bounds(ref, bf16=False):
    """name -> (rtol, atol).  Parameter gradients: rtol 1e-3, atol 1e-4 max|ref| + 1e-5.  A
    stored bf16 element (y, gx with bf16=True): 2^-8 |ref| + the fp32 atol; everything fp32
    keeps the fp32 bound.  bf16 keeps 8 significant bits, so one round to nearest is off by up
    to half an ulp = 2^-8 of the binade's lower end: 2^-8 |ref| is reached (just not
    exceeded) by correct rounding alone, and the fp32 atol is all the room the arithmetic in
    front of the store has."""
    b = {}
    for n, r in ref.items():
        if n in FP32:
            rtol, atol = FP32[n]
            b[n] = (2.0 ** -8, atol) if bf16 and n != "stats" else (rtol, atol)
        else:
            b[n] = (1e-3, 1e-4 * float(r.abs().max()) + 1e-5)
    return b


def worst(got, ref, rtol, atol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 is assert_allclose's condition; inf if
    got holds a NaN or an infinity."""
    got = np.asarray(got, np.float64).reshape(np.shape(ref))
    ref = np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


def ratios(got, ref, bf16=False):
    """name -> error / bound for every tensor of the reference."""
    b = bounds(ref, bf16)
    return {n: worst(got[n], ref[n], *b[n]) for n in ref}


def show(case, what, r):
    print("RATIO", case_id(case), what, " ".join(f"{n}={v:.3g}" for n, v in r.items()))
