"""Cases, inputs, oracle, wrong variants and comparator shared by test_stream_oracle.py (CPU)
and test_gpu_stream_alone.py (GPU); no tests here.

A case is a tuple

    (M, N, L, B, H, C, norm, mask, blocks, calls, pos0)

M streams, N encoder channels, frame length L (stride L/2), bottleneck B, block width H, C
speakers, norm "cLN" | "BN" (the blocks' norms: the separator's first norm is always cLN),
mask "relu" | "softmax" | "identity", blocks = ((P, dil), ...) one entry per TemporalBlock (P
is one number per case: the C ABI fixes it per descriptor and leaves dil free per block),
calls = the frame counts K of the successive calls, pos0 = the stream position of the first
call's first frame.

The oracle is the whole-signal causal forward in plain torch at the dtype it is given (float64
is the reference, float32 the yardstick of test_stream_oracle.py), restated from the reference
model's formulas as oracle/ctn_oracle.py cites them: encoder (conv_tasnet.py:108-117), cLN
(:319-329), eval BatchNorm1d (:300-303), PReLU (:218, 253), the causal depthwise conv with
Chomp1d (:176, 247-250, 289), the mask nonlinearities (:202-207), the decoder (:128-142) and
overlap_and_add (utils.py:9-46).  It knows nothing of chunks, rings or calls and returns every
tensor the per-stage C entries expose, over all frames of the signal:

    w [M,Kt,N]  x0 [M,Kt,B]  ring{i} [M,Kt,H]  y{i} [M,Kt,B]  frames [M,C,Kt,L]
    out [M,C,Kt*S+S]  tail [M,C,Kt,S]   (tail[:, :, k]: what a call ending with frame k carries)

Cutting these at the call boundaries is the tests' job (spans).  With pos0 > 0 the signal has a
prefix of pre = max (P-1)*dil frames: the test loads the prefix's norm-1 rows into the ring
slots (pos0 - i) & (R-1), the prefix's last overlap half into tail_in, and makes its first call
at pos = pos0; expected are the oracle's frames after the prefix.

`wrong=` selects a named wrong variant (WRONG below): what a kernel with one specific defect
would compute.  Those variants do know of calls and rings; the right oracle does not.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from layers_cases import FP32, worst

EPS = 1e-8          # conv_tasnet.py:10
BN_EPS = 1e-5       # nn.BatchNorm1d
QUIET = 1e-3        # amplitude of the quiet frames (cLN variance near EPS)
POISON = 1e30       # samples past the needed length
RTOL, ATOL = FP32["y"]

NORMS = ("cLN", "BN")
MASKS = ("relu", "softmax", "identity")


def case_id(c):
    M, N, L, B, H, C, norm, mask, blocks, calls, pos0 = c
    b = ".".join(f"{p}x{d}" for p, d in blocks)
    k = ".".join(str(v) for v in calls) if len(calls) <= 6 else f"{len(calls)}calls{sum(calls)}"
    return f"M{M}-N{N}-L{L}-B{B}-H{H}-C{C}-{norm}-{mask}-{b}-K{k}-pos{pos0}"


def mk(M=2, N=12, L=4, B=10, H=14, C=2, norm="cLN", mask="relu", blocks=((3, 1), (3, 2)), calls=(5, 9, 1, 8),
       pos0=0):
    return (M, N, L, B, H, C, norm, mask, tuple(blocks), tuple(calls), pos0)


# ----------------------------------------------------------------------------
# the case tables (ctn_stream.hip: ST_NT = 256 threads, 8 frames per workgroup, 4 in the v5
# decode, column chunks of SC_W = 8 | 32 outputs with 256 / SC_W input slices)
# ----------------------------------------------------------------------------
BASE = mk()
# one column chunk short / exact / one over, for both widths; a second trip of the j += 256
# loops (257, 300); fewer inputs than input slices (1, 7); every tail of the 16-unroll
COLUMN_CASES = ([mk(H=H) for H in (1, 7, 8, 9, 31, 32, 33, 40, 255, 256, 257, 300)]
                + [mk(B=B) for B in (1, 8, 9, 33, 40)]
                + [mk(N=N) for N in (1, 9, 33, 257)])
# sc_width(): M * K <= 128 -> 8 columns per workgroup, else 32
WIDTH_CASES = [mk(M=8, calls=(16, 16)), mk(M=3, calls=(43, 43))]
GROUP_CASES = [mk(calls=(1, 7, 8, 9, 16, 17, 3, 4, 5)), mk(calls=(1,) * 12), mk(calls=(1,) * 12, mask="softmax", C=3)]
LONG = (8, 5, 16, 8, 17, 8, 8, 8, 16, 8)          # 102 frames > (8 - 1) * 12
TAP_CASES = ([mk(blocks=((P, 1), (P, 3), (P, 12)), calls=LONG) for P in (1, 2, 3, 5, 8)]
             + [mk(M=1, blocks=((P, 2), (P, 64)), calls=(8, 64, 64, 9, 64, 8)) for P in (2, 3)]
             + [mk(M=1, blocks=((8, 64),), calls=(64,) * 9)])        # R = 7 * 64 + 64 = 512 exactly
# R == (P-1)*dil + K exactly, several wraps; run again with R four times larger (RMUL)
RING_CASES = [mk(blocks=((3, 12),), calls=(8,) * 13), mk(blocks=((3, 4),), calls=(8,) * 7)]
POS_CASES = [mk(blocks=b, calls=(3, 4, 8), pos0=p) for p in (2 ** 31 - 5, 2 ** 32 - 5)
             for b in (((3, 1), (3, 2)), ((3, 12),))]
ONE = ((3, 1),)     # the softmax cases are shallow: scores of +-100 multiply what the blocks leave
CODEC_CASES = ([mk(L=L) for L in (2, 4, 16, 40, 64)]
               + [mk(C=C) for C in (1, 2, 3, 8)]
               + [mk(C=C, mask="softmax", blocks=ONE) for C in (1, 2, 3, 8)]
               + [mk(M=M) for M in (1, 2, 5)]
               + [mk(mask="identity"), mk(mask="identity", C=3, L=16)]
               + [mk(norm="BN", mask=m, blocks=ONE if m == "softmax" else BASE[8]) for m in MASKS]
               + [mk(norm="BN", H=7, B=9, N=33, L=16, C=3)])
CLN7 = mk(H=7)      # the case of the cLN variants: seven channels per block norm
ALL_CASES = list(dict.fromkeys([BASE] + COLUMN_CASES + WIDTH_CASES + GROUP_CASES + TAP_CASES + RING_CASES
                               + POS_CASES + CODEC_CASES))
DETERMINISM_CASE = mk(H=33, B=9, C=3, mask="softmax", blocks=((3, 1), (3, 2)), calls=(5, 9, 8))

# wrong variant -> (the case meant to catch it, tensors it must break, tensors it must leave alone)
WRONG = {
    "tap_reads_stale_before_start": (BASE, ("y0", "y1", "out"), ("w", "x0", "ring0")),
    "tap_order_reversed": (BASE, ("y0", "y1", "out"), ("w", "x0", "ring0")),
    "cln_eps_outside_sqrt": (CLN7, ("x0", "out"), ("w",)),
    "cln_unbiased_var": (CLN7, ("x0", "ring0", "y0", "out"), ("w",)),
    "drop_last_column_chunk_8": (mk(B=9), ("x0", "y1", "out"), ("w",)),
    "drop_last_column_chunk_32": (mk(B=33), ("x0", "y1", "out"), ("w",)),
    "drop_last_partial_frame_group_8": (GROUP_CASES[0], ("frames", "out", "tail"), ("w", "x0", "ring1", "y1")),
    "drop_last_partial_frame_group_4": (GROUP_CASES[0], ("frames", "out", "tail"), ("w", "x0", "ring1", "y1")),
    "ola_zero_tail_at_call_start": (GROUP_CASES[1], ("out",), ("w", "x0", "ring1", "y1", "frames", "tail")),
    "softmax_no_max": (mk(C=3, mask="softmax", blocks=ONE), ("frames", "out", "tail"), ("w", "x0", "ring0", "y0")),
    "ring_slot_mod_need": (BASE, ("ringimage1",), ()),
}
FEW_ELEMENTS = ("tap_reads_stale_before_start", "cln_eps_outside_sqrt", "drop_last_partial_frame_group_8",
                "drop_last_partial_frame_group_4", "ola_zero_tail_at_call_start")


# ----------------------------------------------------------------------------
# geometry
# ----------------------------------------------------------------------------
def pre_frames(case):
    """Frames of prefix in front of the first call: 0 at a stream start."""
    return max((P - 1) * d for P, d in case[8]) if case[10] else 0


def total_frames(case):
    return pre_frames(case) + sum(case[9])


def spans(case):
    """[(k0, K, pos)]: the oracle frame index, frame count and stream position of every call."""
    k0, out = pre_frames(case), []
    for K in case[9]:
        out.append((k0, K, case[10] + k0 - pre_frames(case)))
        k0 += K
    return out


def ring_frames(case, i, rmul=1):
    """The tightest ring the ABI allows for block i, times rmul."""
    P, d = case[8][i]
    need = (P - 1) * d + max(case[9])
    return (1 << max(0, (need - 1).bit_length())) * rmul


def ring_sentinel(M, R, H):
    """Finite, non-zero and distinct per slot: -(3 + slot) - j / 4 in fp32."""
    return -(3.0 + torch.arange(R, dtype=torch.float32).view(1, R, 1)
             + 0.25 * (torch.arange(H, dtype=torch.float32) % 3).view(1, 1, H)).expand(M, R, H).contiguous()


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _seed(case):
    s = 4242
    flat = list(case[:6]) + [NORMS.index(case[6]), MASKS.index(case[7])] + [v for b in case[8] for v in b] \
        + list(case[9]) + [case[10] % 1000003]
    for v in flat:
        s = (s * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return s


def _rms(t):
    return float(t.double().square().mean().sqrt())


@functools.lru_cache(maxsize=None)
def make_inputs(case):
    """-> dict of fp32 tensors in the reference model's orientations (Conv1d weights [out][in]):
    samples [M,T], U [N,L], g0 b0 [N], wb [B,N], blocks [{w1 [H,B], a1 [1], n1, wd [H,P], a2 [1],
    n2, w2 [B,H]}], wm [C*N,B], V [L,N]; a norm is {gamma, beta} (cLN) or {weight, bias, mean,
    var} (BN running statistics).  U, wb, V (and wm of the softmax cases) are rescaled after a
    float64 pass so that w, x0 and the frames have rms 1 and the softmax scores reach +120."""
    M, N, L, B, H, C, norm, mask, blocks, calls, pos0 = case
    S, Kt = L // 2, total_frames(case)
    g = torch.Generator().manual_seed(_seed(case))

    def rn(*s):
        return torch.randn(*s, generator=g)

    def ru(*s):
        return torch.rand(*s, generator=g)

    def sgn(*s):
        return 2.0 * torch.randint(0, 2, s, generator=g) - 1.0

    def affine(n, kind):
        scale, shift = 1.0 + 0.3 * (2 * ru(n) - 1), sgn(n) * (0.2 + 0.3 * ru(n))    # |shift| in [0.2, 0.5]
        if kind == "cLN":
            return {"gamma": scale, "beta": shift}
        return {"weight": scale, "bias": shift, "mean": 0.3 * rn(n), "var": 0.5 + 1.5 * ru(n)}

    def alpha():
        return (0.15 + 0.2 * ru(1)) * (1.0 if float(ru(1)) < 0.75 else -1.0)          # away from 0 and 1

    samples = rn(M, (Kt - 1) * S + L)
    if Kt >= 6:     # frames 2 and 3 of the signal lie wholly inside a quiet stretch
        samples[:, 2 * S:3 * S + L] *= QUIET
    inp = {"samples": samples, "U": rn(N, L) / L ** 0.5, "wb": rn(B, N) / N ** 0.5}
    n0 = affine(N, "cLN")
    inp["g0"], inp["b0"] = n0["gamma"], n0["beta"]
    inp["blocks"] = []
    for P, d in blocks:
        inp["blocks"].append({"w1": rn(H, B) / B ** 0.5, "a1": alpha(), "n1": affine(H, norm),
                              "wd": rn(H, P) / P ** 0.5, "a2": alpha(), "n2": affine(H, norm),
                              "w2": 0.5 * rn(B, H) / H ** 0.5})
    inp["wm"] = rn(C * N, B) / B ** 0.5
    inp["V"] = rn(L, N) / N ** 0.5
    # rescale from float64 passes; every factor is applied to the fp32 weight, so the oracle and
    # the kernels read the same numbers
    loud = torch.ones(Kt, dtype=torch.bool)
    if Kt >= 6:
        loud[2:4] = False
    ref = oracle(case, inp)
    inp["U"] = inp["U"] / _rms(ref["w"][:, loud])
    ref = oracle(case, inp)
    inp["wb"] = inp["wb"] / _rms(ref["x0"])
    if mask == "softmax":
        ref = oracle(case, inp)
        inp["wm"] = inp["wm"] * (120.0 / float(ref["score"].max()))
    ref = oracle(case, inp)
    inp["V"] = inp["V"] / _rms(ref["frames"])
    return inp


def fold_norm(n):
    """The (a, b) pair the kernels take, as streaming._norm_pair makes it: cLN -> (gamma,
    beta), eval BatchNorm -> running scale and shift, in fp32."""
    if "gamma" in n:
        return n["gamma"].contiguous(), n["beta"].contiguous()
    scale = n["weight"] / torch.sqrt(n["var"] + BN_EPS)
    return scale.contiguous(), (n["bias"] - n["mean"] * scale).contiguous()


# ----------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------
def _cln(y, gamma, beta, wrong):
    """conv_tasnet.py:319-329 on [M, C, K]."""
    mean = torch.mean(y, dim=1, keepdim=True)
    var = torch.var(y, dim=1, keepdim=True, unbiased=False)
    g, b = gamma.view(1, -1, 1), beta.view(1, -1, 1)
    if wrong == "cln_unbiased_var":
        var = var * y.shape[1] / (y.shape[1] - 1)
    if wrong == "cln_eps_outside_sqrt":
        return g * (y - mean) / (torch.pow(var, 0.5) + EPS) + b
    return g * (y - mean) / torch.pow(var + EPS, 0.5) + b


def _norm(y, n, dtype, wrong):
    if "gamma" in n:
        return _cln(y, n["gamma"].to(dtype), n["beta"].to(dtype), wrong)
    return F.batch_norm(y, n["mean"].to(dtype), n["var"].to(dtype), n["weight"].to(dtype), n["bias"].to(dtype),
                        False, 0.0, BN_EPS)


def _rows(t):
    return t.transpose(1, 2).contiguous()


def oracle(case, inp, dtype=torch.float64, wrong=None):
    """The whole signal through the causal model in `dtype` -> {name: tensor} (module docstring),
    plus "score" [M,C,N,Kt], the mask conv's output (not compared: the input conditions)."""
    M, N, L, B, H, C, norm, mask, blocks, calls, pos0 = case
    S = L // 2

    def t(v):
        return v.to(dtype)

    if wrong and wrong.startswith("drop_last_column_chunk") or wrong and wrong.startswith("drop_last_partial"):
        wrong, width = wrong.rsplit("_", 1)[0], int(wrong.rsplit("_", 1)[1])
    out = {}
    w = F.relu(F.conv1d(t(inp["samples"]).unsqueeze(1), t(inp["U"]).unsqueeze(1), stride=S))     # [M, N, Kt]
    Kt = w.shape[2]
    assert Kt == total_frames(case)
    out["w"] = _rows(w)
    x = F.conv1d(_cln(w, t(inp["g0"]), t(inp["b0"]), wrong), t(inp["wb"]).unsqueeze(2))
    if wrong == "drop_last_column_chunk":       # the bottleneck's last, partial chunk never written
        x = x.clone()
        x[:, B // width * width:] = 0.0
    out["x0"] = _rows(x)
    for i, ((P, d), b) in enumerate(zip(blocks, inp["blocks"])):
        h = F.conv1d(x, t(b["w1"]).unsqueeze(2))
        h = _norm(F.prelu(h, t(b["a1"])), b["n1"], dtype, wrong)
        out[f"ring{i}"] = _rows(h)
        wd, pad = t(b["wd"]).unsqueeze(1), (P - 1) * d
        if wrong == "tap_order_reversed":
            wd = wd.flip(2)
        if wrong == "tap_reads_stale_before_start" and pad:
            assert pos0 == 0
            R = ring_frames(case, i)
            stale = ring_sentinel(M, R, H)[:, [(s - pad) & (R - 1) for s in range(pad)]]        # [M, pad, H]
            h = F.conv1d(torch.cat([t(stale).transpose(1, 2), h], 2), wd, dilation=d, groups=H)
        else:
            h = F.conv1d(h, wd, padding=pad, dilation=d, groups=H)[:, :, :Kt]                   # Chomp1d(pad)
        h = _norm(F.prelu(h, t(b["a2"])), b["n2"], dtype, wrong)
        x = F.conv1d(h, t(b["w2"]).unsqueeze(2)) + x
        out[f"y{i}"] = _rows(x)
    score = F.conv1d(x, t(inp["wm"]).unsqueeze(2)).view(M, C, N, Kt)
    out["score"] = score
    if mask == "softmax":
        if wrong == "softmax_no_max":
            e = torch.exp(score)
            m = e / e.sum(1, keepdim=True)
        else:
            m = F.softmax(score, dim=1)
    else:
        m = F.relu(score) if mask == "relu" else score
    src = (w.unsqueeze(1) * m).transpose(2, 3)                          # [M, C, Kt, N]
    frames = torch.matmul(src, t(inp["V"]).t())                         # [M, C, Kt, L]
    if wrong == "drop_last_partial_frame_group":
        frames = frames.clone()
        for k0, K, _ in spans(case):
            frames[:, :, k0 + K // width * width:k0 + K] = 0.0
    out["frames"] = frames
    ola = frames.new_zeros(M, C, Kt * S + S)                            # utils.py:9-46 with L = 2 S
    ola[:, :, :Kt * S] += frames[..., :S].reshape(M, C, Kt * S)
    ola[:, :, S:] += frames[..., S:].reshape(M, C, Kt * S)
    if wrong == "ola_zero_tail_at_call_start":
        for k0, K, _ in spans(case):
            if k0:
                ola[:, :, k0 * S:(k0 + 1) * S] -= frames[:, :, k0 - 1, S:]
    out["out"] = ola
    out["tail"] = frames[..., S:].contiguous()
    return out


@functools.lru_cache(maxsize=None)
def reference(case):
    return oracle(case, make_inputs(case))


# ----------------------------------------------------------------------------
# ring images
# ----------------------------------------------------------------------------
def ring_start(case, ref, i, rmul=1):
    """Block i's ring before the first call: the sentinel, and at a mid-stream start the
    prefix's norm-1 rows in the slots (pos0 - j) & (R-1) -> fp32 [M, R, H]."""
    M, H, pos0 = case[0], case[4], case[10]
    R, pre = ring_frames(case, i, rmul), pre_frames(case)
    ring = ring_sentinel(M, R, H).clone()
    for j in range(min(pre, R), 0, -1):
        ring[:, (pos0 - j) & (R - 1)] = ref[f"ring{i}"][:, pre - j].float()
    return ring


def ring_image(case, ref, i, ncalls, rmul=1, wrong=None):
    """What block i's ring holds after the first `ncalls` calls -> float64 [M, R, H]."""
    P, d = case[8][i]
    R = ring_frames(case, i, rmul)
    ring = ring_start(case, ref, i, rmul).double()
    for k0, K, pos in spans(case)[:ncalls]:
        for f in range(K):
            slot = (pos + f) % ((P - 1) * d + K) if wrong == "ring_slot_mod_need" else (pos + f) & (R - 1)
            ring[:, slot] = ref[f"ring{i}"][:, k0 + f]
    return ring


# ----------------------------------------------------------------------------
# the comparator: per element |got - ref| <= ATOL + RTOL |ref|, the project's fp32 numbers
# ----------------------------------------------------------------------------
def ratio(got, ref):
    """max |got - ref| / (ATOL + RTOL |ref|); inf if got is not finite."""
    return worst(got, ref, RTOL, ATOL)


def ratios(got, ref):
    return {n: ratio(got[n], ref[n]) for n in got if n in ref and n != "score"}


def rel(a, b):
    """The whole-tensor L2 figure tests/test_gpu_streaming.py uses (reported, never asserted)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def show(case, what, r):
    print("RATIO", case_id(case), what, " ".join(f"{n}={v:.3g}" for n, v in r.items()))
