#!/usr/bin/env python3
"""What does windowed separation of a long recording cost, stage by stage?  

A --minutes recording at 8 kHz (default 10 minutes) is separated with the paper model in
windows of W = 32000 samples with overlap O = 16000 (C = 2).  Timed on the device, each stage
alone, device events around --reps back-to-back calls, median of three such windows:

  frame_ms        ctn_stitch_frame: the [J, W] windows of the mixture
  forward_ms      the model on all J windows, --batch at a time (bf16 autocast unless --fp32)
  plan_ms         ctn_stitch_plan: correlation, permutation search and chain scan
  ola_ms          ctn_stitch_ola: the permuted cross-fade overlap-add
  torch_stitch_ms the same stitch written with plain torch (unfold, einsum, argmax over the
                  permutation table, the chain as a loop on the host, gather and cat): the baseline
  stitch_gbs      bytes the stitch stage has to move, (2 J C W + C T) 4, over plan_ms + ola_ms,
                  beside copy_peak_gbs, bench.py's measured device-copy ceiling

and prints one JSON object.  Needs a GPU: there is no CPU figure.

    python tools/bench_longform.py [--minutes 10 --batch 8 --reps 20] [--fp32] [--no-forward] [--no-copy-peak]
"""
import argparse
import ctypes
import itertools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conv-tasnet_amd")]

import ctn_lib as L  # noqa: E402
import longform  # noqa: E402

SR, W, O, C = 8000, 32000, 16000, 2


def timed(fn, reps):
    """Median over three windows of `reps` calls each, in ms per call (device events)."""
    for _ in range(3):
        fn()
    windows = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / reps)
    return statistics.median(windows), windows


def torch_stitch(P, T, fade):
    """The stitch in plain torch; the chain runs on the host, as a straightforward version would."""
    J, Cn, Wn = P.shape
    Hs = Wn - O
    S = torch.einsum("jau,jbu->jab", P[:-1, :, Hs:].double(), P[1:, :, :O].double())
    tbl = torch.tensor(list(itertools.permutations(range(Cn))), device=P.device)           # [C!, C]
    scores = S[:, torch.arange(Cn, device=P.device)[None, :], tbl].sum(-1)                  # [J-1, C!]
    perm = tbl[scores.argmax(1)].cpu()
    sigma = [torch.arange(Cn)]
    for j in range(J - 1):
        sigma.append(perm[j][sigma[-1]])
    sigma = torch.stack(sigma).to(P.device)
    Ps = P.gather(1, sigma[:, :, None].expand(-1, -1, Wn))
    head = (1.0 - fade) * Ps[:-1, :, Hs:] + fade * Ps[1:, :, :O]
    seg = torch.cat([head, Ps[1:, :, O:Hs]], dim=-1).permute(1, 0, 2).reshape(Cn, -1)
    return torch.cat([Ps[0, :, :Hs], seg, Ps[-1, :, Hs:]], dim=-1)[:, :T], sigma


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--batch", type=int, default=8, help="windows per forward")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window of the stitch stages")
    ap.add_argument("--fp32", action="store_true", help="fp32 activations (default: bf16 autocast, as bench.py)")
    ap.add_argument("--no-forward", action="store_true", help="skip the model: stitch random windows")
    ap.add_argument("--no-copy-peak", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_longform.py measures on the GPU; none is visible")
    dev = torch.device("cuda")
    lib = L.load()
    T = int(round(a.minutes * 60 * SR))
    J = longform.window_count(T, W, O)
    g = torch.Generator().manual_seed(0)
    x = (0.1 * torch.randn(T, generator=g)).to(dev)
    out = {"minutes": a.minutes, "T": T, "W": W, "O": O, "C": C, "J": J, "batch": a.batch,
           "dtype": "fp32" if a.fp32 else "bf16"}

    out["frame_ms"], out["frame_ms_windows"] = timed(lambda: longform.frame(x, W, O), a.reps)
    win = longform.frame(x, W, O)
    if a.no_forward:
        P = 0.1 * torch.randn(J, C, W, device=dev)
    else:
        import conv_tasnet as ct
        torch.manual_seed(0)
        model = ct.ConvTasNet(256, 20, 256, 512, 3, 8, 4, C).to(dev).eval()
        sep = longform.ChunkedSeparator(model, W, O, batch=a.batch)

        def forward():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=not a.fp32):
                return sep.forward_windows(win)
        out["forward_ms"], out["forward_ms_windows"] = timed(forward, 1)
        P = forward()

    d = L.StitchDesc(J=J, C=C, W=W, O=O, T=T)
    st = L.stream_handle(dev)
    nbytes = lib.ctn_stitch_workspace_bytes(ctypes.byref(d))
    ws = L.workspace(nbytes, dev)
    sim = torch.empty((J, C, C), dtype=torch.float64, device=dev)
    perm, sigma = (torch.empty((J, C), dtype=torch.int32, device=dev) for _ in range(2))
    status = torch.empty((J,), dtype=torch.int32, device=dev)
    res = torch.empty((C, T), dtype=torch.float32, device=dev)
    fade = torch.from_numpy(longform.fade_table(O, "linear")).to(dev)

    def plan():
        L.check(lib.ctn_stitch_plan(ctypes.byref(d), L.ptr(P), L.ptr(sim), L.ptr(perm), L.ptr(sigma), L.ptr(status),
                                    L.ptr(ws), nbytes, st), "ctn_stitch_plan")

    def ola():
        L.check(lib.ctn_stitch_ola(ctypes.byref(d), L.ptr(P), L.ptr(sigma), L.ptr(fade), L.ptr(res), st),
                "ctn_stitch_ola")
    out["plan_ms"], out["plan_ms_windows"] = timed(plan, a.reps)
    out["ola_ms"], out["ola_ms_windows"] = timed(ola, a.reps)
    out["stitch_ms"], out["stitch_ms_windows"] = timed(lambda: (plan(), ola()), a.reps)
    out["torch_stitch_ms"], out["torch_stitch_ms_windows"] = timed(lambda: torch_stitch(P, T, fade), max(a.reps // 4, 1))
    ref, ref_sigma = torch_stitch(P, T, fade)
    out["sigma_equal_torch"] = bool(torch.equal(ref_sigma.int(), sigma))
    out["max_abs_diff_vs_torch"] = float((ref - res).abs().max())
    out["workspace_bytes"] = nbytes
    out["stitch_bytes"] = (2 * J * C * W + C * T) * 4
    out["stitch_gbs"] = out["stitch_bytes"] / (out["stitch_ms"] * 1e-3) / 1e9
    out["plan_gbs"] = 2 * (J - 1) * C * O * 4 / (out["plan_ms"] * 1e-3) / 1e9          # the overlaps, once
    out["ola_gbs"] = (J * C * W + C * T) * 4 / (out["ola_ms"] * 1e-3) / 1e9             # every window + the output
    if not a.no_copy_peak:
        import bench
        out["copy_peak_gbs"], out["copy_peak_by"] = bench.copy_peak_gbs(dev, lib, sizes_mib=(256,), reps=5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
