#!/usr/bin/env python3
"""STOI / ESTOI on the device against the host restatement on one MI355X:
evaluate.cal_STOI_batch for M utterances of T samples at --fs with C speakers (E = C + 1
signals per utterance: the estimates and the mixture), device events, median of three
windows of --reps calls after a warm-up; the host stoi.stoi_details over the same 2 C pairs
per utterance, once in this process and once over --procs worker processes (started before
the GPU is initialised, warm before they are timed); and the paper model's forward of the
same batch as evaluate.py runs it (fp32, no_grad) and under bf16 autocast as bench.py does.
speech_like references, estimates 0.9 s_c + 0.15 (others) + noise.  Prints one JSON object.

    python tools/bench_stoi.py [--M 8 32 --C 2 --T 32000 --fs 8000 --reps 10] [--no-host] [--no-forward]
"""
import argparse
import json
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

import stoi  # noqa: E402
import synthetic  # noqa: E402


def signals(M, C, T):
    mix, src = synthetic.speech_like(M, C, T, 0)
    rng = np.random.default_rng(1)
    mixing = torch.full((C, C), 0.15) + 0.75 * torch.eye(C)
    est = torch.einsum("ec,mct->met", mixing, src)
    est = est + 0.05 * est.std(-1, keepdim=True) * torch.from_numpy(rng.standard_normal(est.shape)).float()
    return src, est, mix


def host_pair(job):
    x, y, fs = job
    r = stoi.stoi_details(x, y, fs)
    return r.stoi, r.estoi


def host_jobs(src, est, mix, fs):
    s, e, x = (t.double().numpy() for t in (src, est, mix))
    M, C, _ = s.shape
    return [(s[m, c], y, fs) for m in range(M) for c in range(C) for y in (e[m, c], x[m])]


def timed(fn, reps):
    """Median over three windows of `reps` calls each, in ms per call (device events)."""
    for _ in range(2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[8, 32], help="batch sizes (utterances)")
    ap.add_argument("--C", type=int, default=2)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--fs", type=int, default=8000)
    ap.add_argument("--reps", type=int, default=10, help="calls per timed window")
    ap.add_argument("--procs", type=int, default=16, help="worker processes of the parallel host run")
    ap.add_argument("--no-host", action="store_true", help="skip the host restatement (profiling runs)")
    ap.add_argument("--no-forward", action="store_true", help="skip the model forward")
    a = ap.parse_args()
    out = {"C": a.C, "T": a.T, "fs": a.fs, "reps": a.reps, "batches": []}
    data = {M: signals(M, a.C, a.T) for M in a.M}
    host = {}
    if not a.no_host:                      # before the GPU is initialised: the workers are forked
        with multiprocessing.get_context("fork").Pool(a.procs) as pool:
            pool.map(host_pair, host_jobs(*signals(a.procs, 1, 4000), a.fs))            # warm
            for M in a.M:
                jobs = host_jobs(*data[M], a.fs)
                t0 = time.perf_counter()
                want = [host_pair(j) for j in jobs]
                t1 = time.perf_counter()
                pool.map(host_pair, jobs, chunksize=max(1, len(jobs) // (4 * a.procs)))
                t2 = time.perf_counter()
                host[M] = (want, 1e3 * (t1 - t0), 1e3 * (t2 - t1))
    if not torch.cuda.is_available():
        sys.exit("bench_stoi.py measures on the GPU; none is visible")
    import evaluate
    for M in a.M:
        src, est, mix = (t.cuda() for t in data[M])
        lengths = torch.full((M,), a.T).cuda()
        row = {"M": M, "pairs": M * (a.C + 1) * a.C}
        row["device_ms"], row["device_ms_windows"] = timed(
            lambda: stoi.stoi_device(src, torch.cat((est, mix.unsqueeze(1)), 1), lengths, a.fs), a.reps)
        t0 = time.perf_counter()
        got = evaluate.cal_STOI_batch(src, est, mix, lengths, a.fs)                      # returns host values
        row["cal_stoi_batch_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        if M in host:
            want, row["host_1_thread_ms"], row["host_procs_ms"] = host[M]
            row["host_procs"] = a.procs
            w = np.asarray(want).reshape(M, a.C, 2, 2)                                   # [m, c, est / mix, stoi / estoi]
            ref = (w[:, :, 0, 0].mean(1), w[:, :, 0, 1].mean(1), w[:, :, 1, 0].mean(1), w[:, :, 1, 1].mean(1))
            row["max_abs_diff"] = float(max(np.abs(g - r).max() for g, r in zip(got, ref)))
            row["host_1_thread_over_device"] = row["host_1_thread_ms"] / row["device_ms"]
            row["host_procs_over_device"] = row["host_procs_ms"] / row["device_ms"]
        if not a.no_forward:
            import conv_tasnet as ct
            torch.manual_seed(0)
            model = ct.ConvTasNet(256, 20, 256, 512, 3, 8, 4, a.C).cuda().eval()
            for name, bf16 in (("forward_fp32_ms", False), ("forward_bf16_ms", True)):
                def forward():
                    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
                        return model(mix)
                row[name], row[name + "_windows"] = timed(forward, 3)
            del model
        out["batches"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
