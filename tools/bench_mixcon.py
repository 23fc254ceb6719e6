#!/usr/bin/env python3
"""Mixture-consistency projection on one MI355X: forward plus backward of
mixture_consistency.mixture_consistency at M x C x T (default 32 x 2 x 32000, the bench
shape's PIT batch, and 16 x 8 x 32000, its mixture-of-mixtures batch with 8 outputs), both
modes, against the same layer written in plain torch (fp32) on the device with autograd.
The bytes the device path moves, counted from the shapes, over its time are set beside the
copy ceiling that bench.py measures.  Device events, median of three windows of --reps calls
after a warm-up.

Every measurement is one step, run in a process of its own under its own time limit; the
first step that fails ends the run.  Prints one JSON object.

    python tools/bench_mixcon.py [--shapes 32x2x32000 16x8x32000 --reps 50]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conv-tasnet_amd")]

EPS = 1e-8
MODES = ("uniform", "power")


def timed(fn, reps):
    """Median over three windows of `reps` calls each, in ms per call (device events)."""
    import torch
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


def batch(M, C, T):
    """Speech-like outputs, a mixture that they miss by a residual, an upstream gradient."""
    import synthetic
    import torch
    _, src = synthetic.speech_like(M, C, T, 0)
    g = torch.Generator().manual_seed(1)
    mix = src.sum(1) + 0.1 * torch.randn(M, T, generator=g)
    grad = torch.randn(M, C, T, generator=g)
    return mix.cuda().contiguous(), src.cuda().contiguous(), torch.full((M,), T).cuda(), grad.cuda()


def moved_bytes(M, C, T, mode):
    """fp32 values the device path reads and writes in forward + backward (no mixture
    gradient): forward C + 1 in, C out; backward C in, C out; power adds the two statistics
    passes (C and 2C + 1 in) and the outputs the element-wise backward reads again (C)."""
    n = (C + 1) + C + C + C
    if mode == "power":
        n += C + (2 * C + 1) + C
    return 4 * n * M * T


def torch_mixcon(x, s, lengths, mode):
    """The definition of DESIGN.md §28 in plain torch (fp32)."""
    import torch
    M, C, T = s.shape
    mask = (torch.arange(T, device=s.device) < lengths.unsqueeze(1)).to(s.dtype).unsqueeze(1)
    r = (x.unsqueeze(1) - s.sum(1, keepdim=True)) * mask
    if mode == "uniform":
        return s + r / C
    p = (s * s * mask).sum(-1, keepdim=True)
    return s + (p + EPS) / (p.sum(1, keepdim=True) + C * EPS) * r


def step_device(a, M, C, T, mode):
    import mixture_consistency as mc
    mix, est, lengths, grad = batch(M, C, T)
    est.requires_grad_(True)

    def fb():
        est.grad = None
        mc.mixture_consistency(mix, est, lengths, mode).backward(grad)
    ms, windows = timed(fb, a.reps)
    nbytes = moved_bytes(M, C, T, mode)
    y = mc.mixture_consistency(mix, est, lengths, mode)
    return {"fwd_bwd_ms": ms, "windows": windows, "bytes_moved": nbytes, "moved_gbs": nbytes / (ms * 1e-3) / 1e9,
            "worst_sum_gap": float((y.sum(1) - mix).abs().max())}


def step_torch(a, M, C, T, mode):
    mix, est, lengths, grad = batch(M, C, T)
    est.requires_grad_(True)

    def fb():
        est.grad = None
        torch_mixcon(mix, est, lengths, mode).backward(grad)
    ms, windows = timed(fb, a.reps)
    y = torch_mixcon(mix, est, lengths, mode)
    return {"fwd_bwd_ms": ms, "windows": windows, "worst_sum_gap": float((y.sum(1) - mix).abs().max())}


def step_copy(a, *_):
    import bench
    import ctn_lib as L
    import torch
    gbs, how = bench.copy_peak_gbs(torch.device("cuda", 0), L.load(), sizes_mib=(512,))
    return {"copy_peak_gbs": gbs, "by": how, "note": "read + write bytes / time"}


STEPS = {"device": step_device, "torch": step_torch, "copy": step_copy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32x2x32000", "16x8x32000"], help="MxCxT")
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--limit", type=int, default=120, help="time limit of one step in seconds")
    ap.add_argument("--step", default=None, help="internal: NAME:MxCxT:MODE, run one step in this process")
    a = ap.parse_args()
    if a.step:
        name, shape, mode = a.step.split(":")
        M, C, T = (int(v) for v in shape.split("x"))
        print("RESULT " + json.dumps(STEPS[name](a, M, C, T, mode)), flush=True)
        return
    out = {"reps": a.reps}
    plan = [(n, sh, mode) for sh in a.shapes for mode in MODES for n in ("device", "torch")] + [("copy", "1x2x1", "-")]
    for name, shape, mode in plan:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step",
               f"{name}:{shape}:{mode}", "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out["failed"] = {"step": f"{name}:{shape}:{mode}", "status": r.returncode, "stderr": r.stderr[-2000:]}
            print(json.dumps(out))
            sys.exit(1)                                  # nothing more is started after a failure
        out["copy" if name == "copy" else f"{name} {shape} {mode}"] = json.loads(lines[0][7:])
    for shape in a.shapes:
        for mode in MODES:
            d, t = out[f"device {shape} {mode}"], out[f"torch {shape} {mode}"]
            out[f"torch_over_device {shape} {mode}"] = t["fwd_bwd_ms"] / d["fwd_bwd_ms"]
            d["share_of_copy_ceiling"] = d["moved_gbs"] / out["copy"]["copy_peak_gbs"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
