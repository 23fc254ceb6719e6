#!/usr/bin/env python3
"""MixIT loss on one MI355X: forward plus backward of
mixit_criterion.cal_mixit_loss at M x C x T (default 16 x {4, 8} x 32000, the mixture-of-
mixtures batch of the bench shape) against (a) the same loss in plain torch on the device,
all 2^C assignments enumerated through a one-hot table and autograd, and (b) the PIT loss
pit_criterion.cal_loss at 2M x 2 x T, the loss the same batch trains with today; the forward
without the remix pass (statistics + search + loss: an upper bound of the statistics pass,
which has no entry of its own) as bytes read per second, at the bench shape and at 16 times
the batch, beside the copy ceiling that bench.py measures.  Device events, median of three
windows of --reps calls after a warm-up.

Every measurement is one step, run in a process of its own under its own time limit; the
first step that fails ends the run.  Prints one JSON object.

    python tools/bench_mixit.py [--M 16 --T 32000 --C 4 8 --reps 20 --mode snr]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conv-tasnet_amd")]

EPS = 1e-8


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
    """Two speech-like sources per recording, C outputs that split them with leakage."""
    import synthetic
    import torch
    _, src = synthetic.speech_like(M, C, T, 0)
    g = torch.Generator().manual_seed(1)
    bits = torch.randint(0, 2, (M, C), generator=g)
    bits[:, 0], bits[:, C - 1] = 0, 1
    onehot = torch.stack((1 - bits, bits), 1).float()                     # [M, 2, C]
    mix = torch.einsum("mnc,mct->mnt", onehot, src)
    est = 0.8 * src + 0.3 * src.std() * torch.randn(src.shape, generator=g)
    return mix.cuda().contiguous(), est.cuda().contiguous(), torch.full((M,), T).cuda()


def torch_mixit(mix, est, lengths, mode, snr_max, table):
    """The definition of DESIGN.md §27 in plain torch: every assignment's remix is formed."""
    import torch
    T = est.size(-1)
    mask = (torch.arange(T, device=est.device) < lengths.unsqueeze(1)).to(est.dtype)[:, None, None, :]
    y = torch.einsum("pnc,mct->mpnt", table, est) * mask                  # [M, 2^C, 2, T]
    x = mix.unsqueeze(1) * mask
    if mode == "snr":
        X = (x * x).sum(-1)
        R = ((x - y) ** 2).sum(-1)
        snr = 10.0 * torch.log10((X + EPS) / (R + 10.0 ** (-snr_max / 10.0) * X + EPS))
    else:
        n = lengths.to(est.dtype)[:, None, None, None]
        xc, yc = (x - x.sum(-1, keepdim=True) / n) * mask, (y - y.sum(-1, keepdim=True) / n) * mask
        D, Et, Ee = (xc * yc).sum(-1), (xc * xc).sum(-1), (yc * yc).sum(-1)
        Pp = D * D * Et / (Et + EPS) ** 2
        Ne = Ee - 2.0 * D * D / (Et + EPS) + Pp
        snr = 10.0 * torch.log10(Pp / (Ne + EPS) + EPS)
    max_snr, assign = snr.mean(-1).max(dim=1)
    return -max_snr.mean(), max_snr, assign


def step_device(a, C):
    import mixit_criterion as mc
    mix, est, lengths = batch(a.M, C, a.T)
    est.requires_grad_(True)

    def fb():
        est.grad = None
        mc.cal_mixit_loss(mix, est, lengths, a.mode, a.snr_max)[0].backward()
    ms, windows = timed(fb, a.reps)
    loss, _, assign, _ = mc.cal_mixit_loss(mix, est, lengths, a.mode, a.snr_max)
    return {"fwd_bwd_ms": ms, "windows": windows, "loss": float(loss), "assign": assign.tolist()}


def step_torch(a, C):
    import torch
    mix, est, lengths = batch(a.M, C, a.T)
    est.requires_grad_(True)
    p = torch.arange(1 << C, device="cuda")
    bits = (p.unsqueeze(1) >> torch.arange(C, device="cuda")) & 1
    table = torch.stack((1 - bits, bits), 1).float()                      # [2^C, 2, C]

    def fb():
        est.grad = None
        torch_mixit(mix, est, lengths, a.mode, a.snr_max, table)[0].backward()
    ms, windows = timed(fb, max(2, a.reps // 4))
    loss, _, assign = torch_mixit(mix, est, lengths, a.mode, a.snr_max, table)
    return {"fwd_bwd_ms": ms, "windows": windows, "loss": float(loss), "assign": assign.tolist()}


def step_pit(a, _C):
    import pit_criterion as pc
    import synthetic
    _, src = synthetic.speech_like(2 * a.M, 2, a.T, 0)
    src = src.cuda()
    est = (0.8 * src + 0.1).contiguous().requires_grad_(True)
    lengths = src.new_full((2 * a.M,), a.T).long()

    def fb():
        est.grad = None
        pc.cal_loss(src, est.clone(), lengths)[0].backward()            # cal_loss masks its input in place

    def clone():
        est.detach().clone()
    ms, windows = timed(fb, a.reps)
    return {"fwd_bwd_ms": ms, "windows": windows, "clone_ms": timed(clone, a.reps)[0], "shape": [2 * a.M, 2, a.T]}


def step_stats(a, C):
    """ctn_mixit_forward without remix: statistics + search + loss."""
    import ctn_lib as L
    import torch
    lib = L.load()
    out = {}
    for scale in (1, 16):
        M = a.M * scale
        mix, est, lengths = batch(a.M, C, a.T)
        mix, est, lengths = mix.repeat(scale, 1, 1), est.repeat(scale, 1, 1), lengths.repeat(scale)
        desc = L.MixitDesc(M, C, a.T, 0, a.snr_max)
        nb = lib.ctn_mixit_workspace_bytes(ctypes.byref(desc))
        ws = L.workspace(nb, "cuda")
        loss, max_snr = torch.empty((), device="cuda"), torch.empty(M, device="cuda")
        assign = torch.empty(M, dtype=torch.int64, device="cuda")
        coef = torch.empty(M, 2, 4, device="cuda")
        stream = L.stream_handle(est.device)

        def fwd():
            L.check(lib.ctn_mixit_forward(ctypes.byref(desc), mix.data_ptr(), est.data_ptr(), lengths.data_ptr(),
                                          loss.data_ptr(), max_snr.data_ptr(), assign.data_ptr(), None,
                                          coef.data_ptr(), ws.data_ptr(), nb, stream), "ctn_mixit_forward")
        ms, windows = timed(fwd, a.reps)
        nbytes = (C + 2) * M * a.T * 4
        out[f"M={M}"] = {"fwd_no_remix_ms": ms, "windows": windows, "bytes_read": nbytes,
                         "read_gbs": nbytes / (ms * 1e-3) / 1e9}
    return out


def step_copy(a, _C):
    import bench
    import ctn_lib as L
    import torch
    gbs, how = bench.copy_peak_gbs(torch.device("cuda", 0), L.load(), sizes_mib=(512,))
    return {"copy_peak_gbs": gbs, "by": how, "note": "read + write bytes / time"}


STEPS = {"device": step_device, "torch": step_torch, "pit": step_pit, "stats": step_stats, "copy": step_copy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=16)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--C", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--mode", default="snr", choices=["snr", "si_snr"])
    ap.add_argument("--snr_max", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--limit", type=int, default=120, help="time limit of one step in seconds")
    ap.add_argument("--step", default=None, help="internal: NAME:C, run one step in this process")
    a = ap.parse_args()
    if a.step:
        name, C = a.step.split(":")
        print("RESULT " + json.dumps(STEPS[name](a, int(C))), flush=True)
        return
    out = {"M": a.M, "T": a.T, "mode": a.mode, "snr_max": a.snr_max, "reps": a.reps}
    plan = [(n, C) for C in a.C for n in ("device", "torch", "stats")] + [("pit", 2), ("copy", 0)]
    for name, C in plan:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", f"{name}:{C}",
               "--M", str(a.M), "--T", str(a.T), "--mode", a.mode, "--snr_max", str(a.snr_max), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            out["failed"] = {"step": f"{name}:{C}", "status": r.returncode, "stderr": r.stderr[-2000:]}
            print(json.dumps(out))
            sys.exit(1)                                  # nothing more is started after a failure
        out[f"{name} C={C}" if name in ("device", "torch", "stats") else name] = json.loads(lines[0][7:])
    for C in a.C:
        out[f"torch_over_device C={C}"] = out[f"torch C={C}"]["fwd_bwd_ms"] / out[f"device C={C}"]["fwd_bwd_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
