#!/usr/bin/env python3
"""Digest of the TemporalBlock's results on fixed inputs, for bit-exact A/B of two libraries.

One TemporalBlock forward + backward per case on fixed seeds; one sha256 per output: y, gx
and the nine parameter gradients (w1, alpha1, gamma1, beta1, wd, alpha2, gamma2, beta2, w2).
The library is the one named by CTN_HIP_LIB, or the in-tree default; run the tool once per
library, in separate processes, and compare the printouts byte for byte:

    python tools/dw_digest.py > a.txt
    CTN_HIP_LIB=/path/to/other/libctn_hip.so python tools/dw_digest.py > b.txt
    cmp a.txt b.txt

The cases are small (a few seconds in all) and each takes a path of the depthwise kernels
and the statistics plumbing: M = 3 ragged utterances of K = 1000 frames (Kp = 1024) through
the wave-item and the lane-group kernels at H = 512; fp32; the separate norm1_bwd kernel;
the finalize launches instead of the folds; several comb items per wave at H = 64 and 128
with P != 3; one BatchNorm block (identity-gLN mode of the kernels).  dw_seg sizes a segment
as rows / resident items, 16 steps at these sizes, so two cLN cases of 48 x 7000 frames add
walks of 83 (forward) and 166 (backward) steps on a 256-CU device: longer than a batch of
63 statistics steps, with a batch boundary, full park flushes and a partial one.
"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

import ctn_lib as L   # noqa: E402
import ctn_ops as ops   # noqa: E402

DEV = "cuda"
NAMES = ["w1", "alpha1", "gamma1", "beta1", "wd", "alpha2", "gamma2", "beta2", "w2"]
# (tag, env, dtype, norm, H, B, P, d, causal[, M, K])
BF, F32 = torch.bfloat16, torch.float32
WAVE = [("gLN", 1, 0), ("gLN", 128, 1), ("cLN", 2, 0), ("cLN", 4, 1)]
CASES = (
    [("wave", {}, BF, n, 512, 256, 3, d, c) for n, d, c in WAVE]
    + [("lanegroup", {"CTN_DW_WAVE": "0"}, BF, n, 512, 256, 3, d, c) for n, d, c in WAVE]
    + [("fp32", {}, F32, "gLN", 512, 256, 3, 4, 0), ("fp32", {}, F32, "cLN", 512, 256, 3, 4, 1)]
    + [("nofuse", {"CTN_FUSE_N1": "0"}, BF, "gLN", 512, 256, 3, 2, 0),
       ("nofuse", {"CTN_FUSE_N1": "0"}, BF, "cLN", 512, 256, 3, 2, 1)]
    + [("nofold", {"CTN_WS_FOLD": "0"}, BF, "gLN", 512, 256, 3, 8, 0)]
    + [("narrow", {}, F32, "gLN", 64, 16, 5, 2, 0), ("narrow", {}, BF, "cLN", 128, 64, 2, 4, 1)]
    + [("bn", {}, F32, "BN", 64, 16, 3, 1, 0)]
    + [("longwalk", {}, BF, "cLN", 512, 256, 3, 1, 1, 48, 7000),
       ("longwalk-lanegroup", {"CTN_DW_WAVE": "0"}, BF, "cLN", 512, 256, 3, 1, 1, 48, 7000)]
)
SWITCHES = ("CTN_DW_WAVE", "CTN_FUSE_N1", "CTN_WS_FOLD")
NORMS = {"gLN": L.NORM_GLN, "cLN": L.NORM_CLN, "BN": L.NORM_BN}


def inputs(seed, M, K, H, B, P):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, B, K, generator=g)
    G = torch.randn(M, B, K, generator=g)
    ps = []
    for n, s in zip(NAMES, [(H, B, 1), (1,), (1, H, 1), (1, H, 1), (H, 1, P), (1,), (1, H, 1), (1, H, 1), (B, H, 1)]):
        if n.startswith("alpha"):
            ps.append(0.25 + 0.05 * torch.randn(1, generator=g))
        elif n.startswith("gamma"):
            ps.append(1.0 + 0.3 * torch.randn(*s, generator=g))
        elif n.startswith("beta"):
            ps.append(0.3 * torch.randn(*s, generator=g))
        else:
            fan = s[1] * s[2] + s[0] * s[2]
            ps.append(torch.randn(*s, generator=g) * (2.0 / fan) ** 0.5)
    return x, G, ps


def run(idx, case):
    tag, env, dtype, norm, H, B, P, d, causal = case[:9]
    M, K = case[9:] or (3, 1000)
    for k in SWITCHES:   # the library reads its switches on every call
        os.environ.pop(k, None)
    os.environ.update(env)
    x_ncw, G, params = inputs(1000 + idx, M, K, H, B, P)
    fr = ops.Frames.of(M, K)
    x = ops.ncw_to_rows(x_ncw.to(DEV), fr, dtype).requires_grad_(True)
    ps = [p.to(DEV).clone().requires_grad_(True) for p in params]
    state = None
    if norm == "BN":
        bns = [torch.nn.BatchNorm1d(H, eps=e).to(DEV) for e in (1e-5, 1e-4)]
        with torch.no_grad():
            for i, bn in enumerate(bns):
                bn.weight.copy_(ps[2 + 4 * i].reshape(H))
                bn.bias.copy_(ps[3 + 4 * i].reshape(H))
                ps[2 + 4 * i], ps[3 + 4 * i] = bn.weight, bn.bias
        state = ops.bn_state(*bns)
    packed = dtype == BF and H == 512
    pack = ops.WeightPacks().get([(ps[0], ps[8])], x.device)[0] if packed else None
    y = ops.TBlockFn.apply(x, fr, (B, H, P, d, bool(causal), NORMS[norm]), pack, state, *ps)
    (ops.rows_to_ncw(y, fr, torch.float32) * G.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    name = f"{tag}-{'bf16' if dtype == BF else 'fp32'}-{norm}-M{M}-K{K}-H{H}-P{P}-d{d}{'c' if causal else 'n'}"
    outs = [("y", y.detach()), ("gx", x.grad)] + [(n, p.grad) for n, p in zip(NAMES, ps)]
    for n, t in outs:
        raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
        print(f"{name} {n} {tuple(t.shape)} {hashlib.sha256(raw).hexdigest()}")


def main():
    np.random.seed(0)
    torch.manual_seed(0)
    for i, c in enumerate(CASES):
        run(i, c)


if __name__ == "__main__":
    main()
