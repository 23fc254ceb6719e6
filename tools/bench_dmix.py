#!/usr/bin/env python3
"""Does the input pipeline keep up with the training step?  

Writes a temporary corpus of PCM16 wav files from synthetic.speech_like (--utts mixtures of
T samples with their C sources, the wsj0-2mix directory layout), then times, per batch of M
utterances, C speakers, T samples:

  dmix_ms          dynamic_mix.DynamicMixer.batch on the device: --steps batches queued back to
                   back and synchronized at the end, median of three such windows
  dmix_speed_ms    the same with speed perturbation (--speeds, default 95 100 105: every source
                   resampled on the device) beside dmix_long_ms, the unperturbed
                   batch on the same corpus: a segment at 105 % needs 1.05 T input samples, which
                   the files of exactly T samples do not hold, so both run on a resident PCM16
                   corpus of --utts / 2 utterances of 2 T samples per speaker (the same bytes)
  host_loader_ms   the training pipeline as train.py builds it: data.AudioDataLoader over the
                   same files, num_workers 0, 4 and 16 — wall time of a pass of --batches
                   minibatches divided by their number (`steady`: from the arrival of the
                   first minibatch, i.e. without the start of the worker processes).  The
                   copy to the device is not included.
  step_ms          bench.py's training step (a child process), for scale
  --aug adds, on the long corpus: dmix_reverb_ms (every source through one of
                   --rirs synthetic room impulse responses of --rir-taps taps), dmix_noise_ms (a
                   noise segment per row from a synthetic pool), dmix_aug_speed_ms (both, with
                   --speeds), and host_fftconvolve_ms: scipy.signal.fftconvolve of the same M * C
                   segments with a response of --rir-taps taps on --fft-threads threads (an fft
                   in fp64, not the library's exact-order direct sum: for scale only)

and prints one JSON object.

    python tools/bench_dmix.py [--M 32 --C 2 --T 32000 --utts 256 --batches 320 --steps 2000] [--no-step | --host-only]
                               [--aug [--rir-taps 4000 --rirs 16]] [--dmix-only]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conv-tasnet_amd"))

import audio_io  # noqa: E402
import data  # noqa: E402
import dynamic_mix  # noqa: E402
import preprocess  # noqa: E402
import synthetic  # noqa: E402

SR = 8000


def write_corpus(root, utts, C, T):
    mix, src = synthetic.speech_like(utts, C, T, 0)
    scale = 0.9 / float(mix.abs().max())                 # inside the PCM16 range
    split = os.path.join(root, "wav", "tr")
    for name in ["mix"] + [f"s{c + 1}" for c in range(C)]:
        os.makedirs(os.path.join(split, name))
    for i in range(utts):
        audio_io.write_wav(os.path.join(split, "mix", f"u{i:05d}.wav"), mix[i].numpy() * scale, SR)
        for c in range(C):
            audio_io.write_wav(os.path.join(split, f"s{c + 1}", f"u{i:05d}.wav"), src[i, c].numpy() * scale, SR)
    out = os.path.join(root, "json", "tr")
    for name in preprocess.speaker_dirs(split):
        preprocess.preprocess_one_dir(os.path.join(split, name), out, name, sample_rate=SR)
    return out


def time_host_loader(json_dir, M, T, workers, batches):
    ds = data.AudioDataset(json_dir, M, sample_rate=SR, segment=T / SR)
    order = [i % len(ds) for i in range(batches)]
    loader = data.AudioDataLoader(torch.utils.data.Subset(ds, order), batch_size=1, num_workers=workers)
    t0 = time.perf_counter()
    first = None
    for mixture, lengths, sources in loader:
        assert mixture.shape == (M, T) and sources.shape[0] == M
        first = first or time.perf_counter()
    end = time.perf_counter()
    return {"ms_per_batch": 1e3 * (end - t0) / batches, "steady_ms_per_batch": 1e3 * (end - first) / (batches - 1)}


def long_corpus(utts, C, T):
    """PCM16 utterances of 2 T samples, utts / 2 per speaker slot, every one its own speaker."""
    _, src = synthetic.speech_like(max(utts // 2, C), C, 2 * T, 1)
    pcm = (src * (0.9 * 32767.0 / float(src.abs().max()))).round().to(torch.int16).numpy()
    waves = [pcm[i, c] for i in range(pcm.shape[0]) for c in range(C)]
    return dynamic_mix.DeviceCorpus(waves, list(range(len(waves))), "cuda")


def aug_pools(a):
    """(RirBank of --rirs synthetic responses of --rir-taps taps, PCM16 noise corpus of 16 x 4 T)."""
    rirs = [synthetic.synthetic_rir(a.rir_taps, 0.4, SR, seed) for seed in range(a.rirs)]
    _, src = synthetic.speech_like(16, 1, 4 * a.T, 2)
    pcm = (src[:, 0] * (0.5 * 32767.0 / float(src.abs().max()))).round().to(torch.int16).numpy()
    return dynamic_mix.RirBank(rirs, "cuda"), dynamic_mix.DeviceCorpus(list(pcm), list(range(len(pcm))), "cuda")


def time_host_fftconvolve(M, C, T, taps, threads):
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np
    from scipy.signal import fftconvolve
    rng = np.random.default_rng(0)
    x, h = rng.standard_normal((M * C, T)), synthetic.synthetic_rir(taps, 0.4, SR, 0).astype(np.float64)
    runs = []
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(5):
            t0 = time.perf_counter()
            list(pool.map(lambda row: fftconvolve(row, h)[:T], x))
            runs.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(runs[1:])


def time_dmix(corpus, M, C, T, steps, speeds=None, **aug):
    mixer = dynamic_mix.DynamicMixer(corpus, M, C, T, speeds=speeds, **aug)
    for step in range(10):
        mixer.batch(step)
    windows = []
    for w in range(3):                                   # three windows of `steps` batches each
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for step in range(steps):
            mixer.batch(10 + w * steps + step)
        torch.cuda.synchronize()
        windows.append(1e3 * (time.perf_counter() - t0) / steps)
    return statistics.median(windows), windows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--C", type=int, default=2)
    ap.add_argument("--T", type=int, default=32000)
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--batches", type=int, default=320, help="minibatches per host-loader pass")
    ap.add_argument("--steps", type=int, default=2000, help="DynamicMixer batches per timed window")
    ap.add_argument("--workers", type=int, nargs="*", default=[0, 4, 16])
    ap.add_argument("--speeds", type=int, nargs="+", default=[95, 100, 105], help="percents of the perturbed row")
    ap.add_argument("--no-step", action="store_true", help="skip the bench.py run")
    ap.add_argument("--host-only", action="store_true", help="time the host loader only (needs no GPU)")
    ap.add_argument("--dmix-only", action="store_true", help="time the device rows only (no host loader, no bench.py)")
    ap.add_argument("--aug", action="store_true", help="add the reverberation and noise rows")
    ap.add_argument("--rir-taps", type=int, default=4000, help="taps of the synthetic room impulse responses")
    ap.add_argument("--rirs", type=int, default=16, help="room impulse responses in the bank")
    ap.add_argument("--fft-threads", type=int, default=16, help="threads of the host fftconvolve figure")
    a = ap.parse_args()
    out ={"M": a.M, "C": a.C, "T": a.T, "utts": a.utts}
    with tempfile.TemporaryDirectory() as root:
        json_dir = write_corpus(root, a.utts, a.C, a.T)
        # the worker processes are forked before this process opens the GPU
        if not a.dmix_only:
            out["host_loader_ms"] = {str(w): time_host_loader(json_dir, a.M, a.T, w, a.batches) for w in a.workers}
        if a.aug:
            out["rir_taps"], out["fft_threads"] = a.rir_taps, a.fft_threads
            out["host_fftconvolve_ms"] = time_host_fftconvolve(a.M, a.C, a.T, a.rir_taps, a.fft_threads)
        if not a.host_only:
            corpus = dynamic_mix.DeviceCorpus.from_json_dir(json_dir, SR, speaker_of=lambda path, slot: (slot, path))
            out["dmix_ms"], out["dmix_ms_windows"] = time_dmix(corpus, a.M, a.C, a.T, a.steps)
            out["corpus_bytes"], out["pool_dtype"] = corpus.nbytes, "int16" if corpus.pool_dtype == 0 else "fp32"
            corpus = long_corpus(a.utts, a.C, a.T)
            out["dmix_long_ms"], out["dmix_long_ms_windows"] = time_dmix(corpus, a.M, a.C, a.T, a.steps)
            out["speeds"] = a.speeds
            out["dmix_speed_ms"], out["dmix_speed_ms_windows"] = time_dmix(corpus, a.M, a.C, a.T, a.steps, a.speeds)
            if a.aug:
                bank, noise = aug_pools(a)
                steps = max(a.steps // 4, 1)
                out["dmix_reverb_ms"], out["dmix_reverb_ms_windows"] = time_dmix(corpus, a.M, a.C, a.T, steps, rirs=bank)
                out["dmix_noise_ms"], out["dmix_noise_ms_windows"] = time_dmix(corpus, a.M, a.C, a.T, a.steps, noise=noise)
                out["dmix_aug_speed_ms"], out["dmix_aug_speed_ms_windows"] = time_dmix(
                    corpus, a.M, a.C, a.T, steps, a.speeds, rirs=bank, noise=noise)
    if not (a.no_step or a.host_only or a.dmix_only):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                           check=True, capture_output=True, text=True)
        out["step_ms"] = json.loads(r.stdout.strip().splitlines()[-1])["ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
