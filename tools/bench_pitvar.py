#!/usr/bin/env python3
"""PIT with silent sources on one MI355X: forward plus backward of
pit_var_criterion.cal_loss_var at M x C x T (default 32 x 2 x 32000 and 16 x 4 x 32000, a
third of the references silent) against (a) the existing PIT loss pit_criterion.cal_loss at the
same shape, the yardstick, (b) the same loss in plain torch on the device, the C x C scores
through a broadcast residual and all C! permutations through a table and autograd, and (c) the
dynamic mixer's batch at the same shape with and without the speaker-count draw
(DynamicMixer(min_speakers=1) against the default).  tools/bench_mixit.py's method: device
events, median of three windows of --reps calls after a warm-up.

Every measurement is one step, run in a process of its own under its own time limit; the
first step that fails ends the run.  Prints one JSON object.

    python tools/bench_pitvar.py [--shapes 32x2 16x4 --T 32000 --reps 20 --mode snr]
"""
import argparse
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "conv-tasnet_amd"), os.path.join(ROOT, "tools")]

from bench_mixit import timed  # noqa: E402

EPS = 1e-8


def batch(M, C, T):
    """Speech-like references, every third one silent (never reference 0), outputs that follow
    them with leakage (quiet where the reference is silent), the mixture with a little noise."""
    import synthetic
    import torch
    _, src = synthetic.speech_like(M, C, T, 0)
    g = torch.Generator().manual_seed(1)
    noise = src.std() * torch.randn(src.shape, generator=g)
    silent = (torch.arange(M * C).reshape(M, C) % 3 == 1) & (torch.arange(C) > 0)
    src[silent] = 0.0
    est = torch.where(silent[:, :, None], 0.05 * noise, 0.8 * src + 0.3 * noise)
    mix = src.sum(1) + 0.1 * noise[:, 0]
    return src.cuda().contiguous(), est.cuda().contiguous(), mix.cuda().contiguous(), torch.full((M,), T).cuda()


def torch_pitvar(src, est, mix, lengths, mode, snr_max, inactive_snr_max, table):
    """The definition of DESIGN.md §29 in plain torch: every residual is formed."""
    import torch
    M, C, T = est.shape
    mask = (torch.arange(T, device=est.device) < lengths.unsqueeze(1)).to(est.dtype)[:, None, :]
    s, e, x = src * mask, est * mask, mix * mask[:, 0]
    S, E, X = (s * s).sum(-1), (e * e).sum(-1), (x * x).sum(-1)
    active = S > 0
    if mode == "snr":
        R = ((s[:, None, :, :] - e[:, :, None, :]) ** 2).sum(-1)            # [M, i, j]
        act = 10.0 * torch.log10((S[:, None, :] + EPS) / (R + 10.0 ** (-snr_max / 10.0) * S[:, None, :] + EPS))
    else:
        n = lengths.to(est.dtype)[:, None, None]
        sc, ec = (s - s.sum(-1, keepdim=True) / n) * mask, (e - e.sum(-1, keepdim=True) / n) * mask
        D = torch.einsum("mit,mjt->mij", ec, sc)
        Et, Ee = (sc * sc).sum(-1)[:, None, :], (ec * ec).sum(-1)[:, :, None]
        Pp = D * D * Et / (Et + EPS) ** 2
        act = 10.0 * torch.log10(Pp / (Ee - 2.0 * D * D / (Et + EPS) + Pp + EPS) + EPS)
    quiet = 10.0 * torch.log10((X[:, None] + EPS) / (E + 10.0 ** (-inactive_snr_max / 10.0) * X[:, None] + EPS))
    scores = torch.where(active[:, None, :], act, quiet[:, :, None].expand(M, C, C))
    sums = scores[:, torch.arange(C, device=est.device)[None, :], table].sum(-1)               # [M, C!]
    max_snr, rank = sums.max(dim=1)
    return -(max_snr / C).mean(), max_snr / C, table[rank], active


def step_device(a, M, C):
    import pit_var_criterion as pv
    src, est, mix, lengths = batch(M, C, a.T)
    est.requires_grad_(True)

    def fb():
        est.grad = None
        pv.cal_loss_var(src, est, lengths, mix, a.mode, a.snr_max, a.inactive_snr_max)[0].backward()
    ms, windows = timed(fb, a.reps)
    loss, _, perm, active = pv.cal_loss_var(src, est, lengths, mix, a.mode, a.snr_max, a.inactive_snr_max)
    return {"fwd_bwd_ms": ms, "windows": windows, "loss": float(loss), "perm0": perm[0].tolist(),
            "active_refs": int(active.sum())}


def step_torch(a, M, C):
    import torch
    src, est, mix, lengths = batch(M, C, a.T)
    est.requires_grad_(True)
    table = torch.tensor(list(itertools.permutations(range(C))), device="cuda")

    def fb():
        est.grad = None
        torch_pitvar(src, est, mix, lengths, a.mode, a.snr_max, a.inactive_snr_max, table)[0].backward()
    ms, windows = timed(fb, max(2, a.reps // 4))
    loss, _, perm, active = torch_pitvar(src, est, mix, lengths, a.mode, a.snr_max, a.inactive_snr_max, table)
    return {"fwd_bwd_ms": ms, "windows": windows, "loss": float(loss), "perm0": perm[0].tolist(),
            "active_refs": int(active.sum())}


def step_pit(a, M, C):
    """The existing PIT kernels at the same shape (all references speaking): the yardstick."""
    import pit_criterion as pc
    import synthetic
    _, src = synthetic.speech_like(M, C, a.T, 0)
    src = src.cuda()
    est = (0.8 * src + 0.1).contiguous().requires_grad_(True)
    lengths = src.new_full((M,), a.T).long()

    def fb():
        est.grad = None
        pc.cal_loss(src, est.clone(), lengths)[0].backward()            # cal_loss masks its input in place

    def clone():
        est.detach().clone()
    ms, windows = timed(fb, a.reps)
    return {"fwd_bwd_ms": ms, "windows": windows, "clone_ms": timed(clone, a.reps)[0]}


def step_mixer(a, M, C):
    """One mixer batch (draw + mix) at M x C x T from a synthetic int16 corpus, with the
    speaker-count draw (min_speakers = 1) and without."""
    import numpy as np

    import dynamic_mix as dm
    rng = np.random.default_rng(0)
    waves = [(rng.standard_normal(a.T + int(rng.integers(1, a.T))) * 3000).astype(np.int16) for _ in range(64)]
    corpus = dm.DeviceCorpus(waves, [u % 16 for u in range(64)], "cuda")
    out = {}
    for name, k in (("all_speak", None), ("thinned", 1)):
        mx = dm.DynamicMixer(corpus, M, C, a.T, seed=1, min_speakers=k)
        step = [0]

        def run():
            step[0] += 1
            mx.batch(step[0])
        ms, windows = timed(run, a.reps)
        out[name] = {"batch_ms": ms, "windows": windows, "mean_count": float(mx.count.float().mean())}
    return out


STEPS = {"device": step_device, "torch": step_torch, "pit": step_pit, "mixer": step_mixer}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["32x2", "16x4"], help="MxC")
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--mode", default="snr", choices=["snr", "si_snr"])
    ap.add_argument("--snr_max", type=float, default=30.0)
    ap.add_argument("--inactive_snr_max", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--limit", type=int, default=120, help="time limit of one step in seconds")
    ap.add_argument("--step", default=None, help="internal: NAME:MxC, run one step in this process")
    a = ap.parse_args()
    if a.step:
        name, shape = a.step.split(":")
        M, C = (int(v) for v in shape.split("x"))
        print("RESULT " + json.dumps(STEPS[name](a, M, C)), flush=True)
        return
    out = {"T": a.T, "mode": a.mode, "snr_max": a.snr_max, "inactive_snr_max": a.inactive_snr_max, "reps": a.reps}
    for shape in a.shapes:
        for name in ("device", "pit", "torch", "mixer"):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step",
                   f"{name}:{shape}", "--T", str(a.T), "--mode", a.mode, "--snr_max", str(a.snr_max),
                   "--inactive_snr_max", str(a.inactive_snr_max), "--reps", str(a.reps)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not lines:
                out["failed"] = {"step": f"{name}:{shape}", "status": r.returncode, "stderr": r.stderr[-2000:]}
                print(json.dumps(out))
                sys.exit(1)                              # nothing more is started after a failure
            out[f"{name} {shape}"] = json.loads(lines[0][7:])
        out[f"torch_over_device {shape}"] = out[f"torch {shape}"]["fwd_bwd_ms"] / out[f"device {shape}"]["fwd_bwd_ms"]
        out[f"device_over_pit {shape}"] = out[f"device {shape}"]["fwd_bwd_ms"] / out[f"pit {shape}"]["fwd_bwd_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
