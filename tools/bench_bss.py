#!/usr/bin/env python3
"""SDRi on the device against the host routine on one MI355X ("BSS Eval on the
device"): evaluate.cal_SDRi_batch for M utterances of T samples with C speakers and
flen-tap filters, synchronized, median of --runs calls after one warm-up, and the host
evaluate.cal_SDRi over the same utterances in the same process.  speech_like references,
estimates 0.9 s_c + 0.15 (others) + noise, the mixture as the anchor.  Prints one JSON object.

    python tools/bench_bss.py [--M 8 --C 2 --T 32000 --flen 512 --runs 5] [--no-host]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

import bss_eval  # noqa: E402
import evaluate  # noqa: E402
import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=8)
    ap.add_argument("--C", type=int, default=2)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--flen", type=int, default=bss_eval.FLEN)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host routine (profiling runs)")
    a = ap.parse_args()
    mix, src = synthetic.speech_like(a.M, a.C, a.T, 0)
    rng = np.random.default_rng(1)
    mixing = torch.full((a.C, a.C), 0.15) + 0.75 * torch.eye(a.C)
    est = torch.einsum("ec,mct->met", mixing, src)
    est = est + 0.05 * est.std(-1, keepdim=True) * torch.from_numpy(rng.standard_normal(est.shape)).float()
    lengths = torch.full((a.M,), a.T)
    dev = [t.cuda() for t in (src, est, mix, lengths)]
    times = []
    for i in range(a.runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = evaluate.cal_SDRi_batch(*dev, flen=a.flen)      # returns host values: synchronized
        times.append(time.perf_counter() - t0)
    out = {"M": a.M, "C": a.C, "T": a.T, "flen": a.flen, "runs": a.runs,
           "device_ms": 1e3 * statistics.median(times[1:]), "device_ms_all": [1e3 * t for t in times]}
    if not a.no_host:
        t0 = time.perf_counter()
        want = []
        for m in range(a.M):
            s, e, x = (t[m].double().numpy() for t in (src, est, mix))
            anchor = np.stack([x] * a.C)
            want.append(float(np.mean(bss_eval.bss_eval_sources(s, e, flen=a.flen)[0] -
                                      bss_eval.bss_eval_sources(s, anchor, flen=a.flen)[0])))
        out["host_ms"] = 1e3 * (time.perf_counter() - t0)
        out["host_over_device"] = out["host_ms"] / out["device_ms"]
        out["max_abs_diff_db"] = float(np.abs(np.asarray(want) - got).max())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
