#!/usr/bin/env python
"""Drop-in for ``src/train.py``: the same flags and
defaults (train.py:15-98) and the same Solver loop, on the HIP path.

    python train.py --train_dir data/tr --valid_dir data/cv ...            # one GPU
    torchrun --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...       # one process per GPU

Differences, each deliberate:
* multi-GPU is one process per GPU (DDP over RCCL, ``nccl`` backend) instead of
  nn.DataParallel (train.py:121): every rank trains its own share of the
  minibatches (data.MinibatchSampler) and DDP averages the gradients; on one
  GPU the model is wrapped in ``Single`` so ``.module`` works as the solver
  expects (solver.py:55,87,131);
* ``--optimizer adam`` is ctn_optim.Adam (torch.optim.Adam's update and
  state_dict, one launch per step); ``sgd`` is torch.optim.SGD;
* ``--shuffle`` reshuffles the minibatch order per epoch through the sampler
  (a DataLoader cannot take both a sampler and shuffle=True);
* ``--bf16 1`` trains with bf16 activations (fp32 parameters, statistics and
  optimizer state); the default 0 is fp32, the reference's arithmetic;
* ``--dynamic_mix 1`` (default 0: the fixed mixtures, as the reference) replaces the
  training loader by dynamic_mix.DynamicMixLoader: batches drawn and mixed on the GPU from
  the s1..sC utterances of --train_dir (``--dm_*`` flags); cross validation is unchanged.
  ``--dm_speeds 95 100 105`` adds speed perturbation: each source is resampled on the GPU to
  one of these speeds before it is mixed.  ``--dm_rir_dir`` / ``--dm_noise_dir`` (directories
  of wav files) add reverberation and noise on the GPU: every source is convolved with a drawn
  room impulse response (probability ``--dm_rir_prob``; responses longer than
  ``--dm_rir_max_taps`` are truncated) and every mixture gets a drawn noise segment at an SNR
  from ``--dm_snr_db LO HI``.  Cross validation keeps the fixed set;
* ``--loss mixit`` (default ``pit``: nothing changes) trains without isolated sources
  (mixit_criterion.py): utterances 2m and 2m+1 of every training batch are
  added into one mixture of mixtures, the model separates it into ``--C`` outputs (2 to 8) and
  the MixIT loss (``--mixit_loss snr|si_snr``, ``--mixit_snr_max``) scores the best remix
  against the two mixtures; ``--batch_size`` must be even.  With ``--dynamic_mix 1`` the mixer
  draws ``--mixit_speakers`` speakers per single mixture.  Cross validation remixes the
  outputs to the two sources of each validation mixture;
* ``--mixture_consistency uniform|power`` (default ``none``: nothing changes) puts the
  mixture-consistency projection on the model's outputs (mixture_consistency.py, DESIGN.md
  §28), with either loss; the mode is written into the package;
* ``--loss pit_var`` (pit_var_criterion.py) trains one model with ``--C`` outputs
  (2 to 8) on mixtures of 1 to C speakers: a source that is all zero is silent, its output is
  scored by how far it lies below the input mixture, and the permutation is searched over
  active and silent sources together (``--var_loss snr|si_snr``, ``--var_snr_max``,
  ``--var_inactive_snr_max``).  ``--dm_min_speakers K`` (default 0: always C) lets the dynamic
  mixer draw how many of a row's slots speak, K to C; it needs ``--loss pit_var`` or ``mixit``,
  because the plain PIT loss scores a silent source as noise.  Cross validation uses the same
  loss on the fixed set, whose silent sources are all-zero files.
"""
import argparse
import os

import torch
import torch.distributed as dist

from conv_tasnet import ConvTasNet
from data import AudioDataLoader, AudioDataset, MinibatchSampler
from solver import Solver

parser = argparse.ArgumentParser(
    "Fully-Convolutional Time-domain Audio Separation Network (Conv-TasNet) "
    "with Permutation Invariant Training")
# Task related
parser.add_argument('--train_dir', type=str, default=None,
                    help='directory including mix.json, s1.json and s2.json')
parser.add_argument('--valid_dir', type=str, default=None,
                    help='directory including mix.json, s1.json and s2.json')
parser.add_argument('--sample_rate', default=8000, type=int,
                    help='Sample rate')
parser.add_argument('--segment', default=4, type=float,
                    help='Segment length (seconds)')
parser.add_argument('--cv_maxlen', default=8, type=float,
                    help='max audio length (seconds) in cv, to avoid OOM issue.')
# Network architecture
parser.add_argument('--N', default=256, type=int,
                    help='Number of filters in autoencoder')
parser.add_argument('--L', default=20, type=int,
                    help='Length of the filters in samples (40=5ms at 8kHZ)')
parser.add_argument('--B', default=256, type=int,
                    help='Number of channels in bottleneck 1 × 1-conv block')
parser.add_argument('--H', default=512, type=int,
                    help='Number of channels in convolutional blocks')
parser.add_argument('--P', default=3, type=int,
                    help='Kernel size in convolutional blocks')
parser.add_argument('--X', default=8, type=int,
                    help='Number of convolutional blocks in each repeat')
parser.add_argument('--R', default=4, type=int,
                    help='Number of repeats')
parser.add_argument('--C', default=2, type=int,
                    help='Number of speakers')
parser.add_argument('--norm_type', default='gLN', type=str,
                    choices=['gLN', 'cLN', 'BN'], help='Layer norm type')
parser.add_argument('--causal', type=int, default=0,
                    help='Causal (1) or noncausal(0) training')
parser.add_argument('--mask_nonlinear', default='relu', type=str,
                    choices=['relu', 'softmax'], help='non-linear to generate mask')
# Training config
parser.add_argument('--use_cuda', type=int, default=1,
                    help='Whether use GPU')
parser.add_argument('--epochs', default=30, type=int,
                    help='Number of maximum epochs')
parser.add_argument('--half_lr', dest='half_lr', default=0, type=int,
                    help='Halving learning rate when get small improvement')
parser.add_argument('--early_stop', dest='early_stop', default=0, type=int,
                    help='Early stop training when no improvement for 10 epochs')
parser.add_argument('--max_norm', default=5, type=float,
                    help='Gradient norm threshold to clip')
# minibatch
parser.add_argument('--shuffle', default=0, type=int,
                    help='reshuffle the data at every epoch')
parser.add_argument('--batch_size', default=128, type=int,
                    help='Batch size')
parser.add_argument('--num_workers', default=4, type=int,
                    help='Number of workers to generate minibatch')
# optimizer
parser.add_argument('--optimizer', default='adam', type=str,
                    choices=['sgd', 'adam'],
                    help='Optimizer (support sgd and adam now)')
parser.add_argument('--lr', default=1e-3, type=float,
                    help='Init learning rate')
parser.add_argument('--momentum', default=0.0, type=float,
                    help='Momentum for optimizer')
parser.add_argument('--l2', default=0.0, type=float,
                    help='weight decay (L2 penalty)')
# save and load model
parser.add_argument('--save_folder', default='exp/temp',
                    help='Location to save epoch models')
parser.add_argument('--checkpoint', dest='checkpoint', default=0, type=int,
                    help='Enables checkpoint saving of model')
parser.add_argument('--continue_from', default='',
                    help='Continue from checkpoint model')
parser.add_argument('--model_path', default='final.pth.tar',
                    help='Location to save best validation model')
# logging
parser.add_argument('--print_freq', default=10, type=int,
                    help='Frequency of printing training infomation')
parser.add_argument('--visdom', dest='visdom', type=int, default=0,
                    help='Turn on visdom graphing')
parser.add_argument('--visdom_epoch', dest='visdom_epoch', type=int, default=0,
                    help='Turn on visdom graphing each epoch')
parser.add_argument('--visdom_id', default='TasNet training',
                    help='Identifier for visdom run')
# MI355X path
parser.add_argument('--bf16', default=0, type=int,
                    help='1: bf16 activations (fp32 parameters, statistics and optimizer state)')
# dynamic mixing on the device (dynamic_mix.py); 0: the corpus's fixed mixtures, as the reference
parser.add_argument('--dynamic_mix', default=0, type=int,
                    help='1: draw and mix every training batch on the GPU from the s1..sC utterances of --train_dir')
parser.add_argument('--dm_seed', default=0, type=int,
                    help='Seed of the dynamic-mixing draws')
parser.add_argument('--dm_level_mode', default=0, type=int, choices=[0, 1],
                    help='0: level on the stored waveform, 1: relative to the segment RMS')
parser.add_argument('--dm_level_db', default=[-2.5, 2.5], type=float, nargs=2, metavar=('LO', 'HI'),
                    help='Range of the uniform per-source level draw (dB)')
parser.add_argument('--dm_peak', default=0.9, type=float,
                    help='Mixtures peaking above this are scaled down to it (0: off)')
parser.add_argument('--dm_steps', default=0, type=int,
                    help='Steps per epoch (0: the number of minibatches the static loader gives this rank)')
parser.add_argument('--dm_speeds', default=[100], type=int, nargs='+', metavar='PCT',
                    help='Speed perturbation: every source is played at one of these percents, drawn per source '
                         '(e.g. 95 100 105; at most 8; the default 100 is off)')
parser.add_argument('--dm_rir_dir', default='', type=str,
                    help='Directory of room impulse responses (wav): every source is convolved with a drawn one '
                         '(default: off)')
parser.add_argument('--dm_rir_prob', default=1.0, type=float,
                    help='Probability that a source is reverberated')
parser.add_argument('--dm_rir_max_taps', default=16384, type=int,
                    help='Longer room impulse responses are truncated to this many taps (at most 16384)')
parser.add_argument('--dm_noise_dir', default='', type=str,
                    help='Directory of noise recordings (wav): every mixture gets a drawn segment (default: off)')
parser.add_argument('--dm_snr_db', default=[-5.0, 5.0], type=float, nargs=2, metavar=('LO', 'HI'),
                    help='Range of the uniform draw of the clean mixture to noise ratio (dB)')

# MixIT (mixit_criterion.py); pit: the reference's loss on isolated sources
parser.add_argument('--loss', default='pit', type=str, choices=['pit', 'mixit', 'pit_var'],
                    help='pit: PIT SI-SNR against the sources.  mixit: mixture-invariant training, every two '
                         'utterances of a batch are added into one mixture of mixtures and --C is the number of '
                         'model outputs; the sources are not used.  pit_var: PIT in which an all-zero source is '
                         'silent and its output is pushed below the mixture (1 to --C speakers per mixture)')
parser.add_argument('--mixit_loss', default='snr', type=str, choices=['snr', 'si_snr'],
                    help='MixIT score: snr (thresholded at --mixit_snr_max) or si_snr')
parser.add_argument('--mixit_snr_max', default=30.0, type=float,
                    help='MixIT soft SNR ceiling in dB (snr only)')
parser.add_argument('--mixit_speakers', default=2, type=int,
                    help='Speakers the dynamic mixer draws per single mixture under --loss mixit')

# PIT with silent sources (pit_var_criterion.py)
parser.add_argument('--var_loss', default='snr', type=str, choices=['snr', 'si_snr'],
                    help='pit_var score of an active source: snr (thresholded at --var_snr_max) or si_snr')
parser.add_argument('--var_snr_max', default=30.0, type=float,
                    help='pit_var soft SNR ceiling of an active source in dB (snr only)')
parser.add_argument('--var_inactive_snr_max', default=20.0, type=float,
                    help='pit_var: an output paired with a silent source is pushed this many dB below the mixture')
parser.add_argument('--dm_min_speakers', default=0, type=int,
                    help='Dynamic mixing: every row keeps a drawn number of its speakers, from this many to all '
                         '(0: always all; needs --loss pit_var or mixit)')

# mixture consistency (mixture_consistency.py); none: the reference's model
parser.add_argument('--mixture_consistency', default='none', type=str, choices=['none', 'uniform', 'power'],
                    help='Project the model outputs so that they add up to the input mixture: the residual is '
                         'spread evenly (uniform) or by output power (power); works with either --loss')


def check_mixture_consistency(args):
    """--mixture_consistency uniform|power needs 2 to 16 model outputs."""
    mode = getattr(args, 'mixture_consistency', 'none')
    if mode not in ('none', 'uniform', 'power'):
        raise ValueError(f"--mixture_consistency {mode}: one of none, uniform, power")
    if mode != 'none' and not 2 <= args.C <= 16:
        raise ValueError(f"--mixture_consistency {mode}: --C {args.C} must be 2 to 16")


def check_mixit(args):
    """--loss mixit pairs the utterances of a batch and needs at least two model outputs."""
    import math
    if args.loss != 'mixit':
        return
    if args.batch_size < 2 or args.batch_size % 2:
        raise ValueError(f"--loss mixit adds utterances 2m and 2m+1 of a batch into one mixture of mixtures: "
                         f"--batch_size {args.batch_size} must be even")
    if not 2 <= args.C <= 8:
        raise ValueError(f"--loss mixit: --C {args.C} is the number of model outputs, 2 to 8")
    if not math.isfinite(args.mixit_snr_max):
        raise ValueError(f"--mixit_snr_max {args.mixit_snr_max}: a finite value in dB")
    if args.mixit_speakers < 1:
        raise ValueError(f"--mixit_speakers {args.mixit_speakers}: at least 1")


def check_var(args):
    """--loss pit_var and --dm_min_speakers: exits with the reason when they cannot work."""
    import math
    loss, k = getattr(args, 'loss', 'pit'), getattr(args, 'dm_min_speakers', 0)
    if loss == 'pit_var':
        if not 2 <= args.C <= 8:
            raise SystemExit(f"--loss pit_var: --C {args.C} is the number of model outputs, 2 to 8")
        if not (math.isfinite(args.var_snr_max) and math.isfinite(args.var_inactive_snr_max)):
            raise SystemExit("--var_snr_max and --var_inactive_snr_max: finite values in dB")
    if k == 0:
        return
    slots = args.mixit_speakers if loss == 'mixit' else args.C
    if not 1 <= k <= slots:
        raise SystemExit(f"--dm_min_speakers {k}: 1 to the {slots} speakers the mixer draws "
                         f"({'--mixit_speakers' if loss == 'mixit' else '--C'}), or 0 for all of them")
    if not args.dynamic_mix:
        raise SystemExit("--dm_min_speakers thins the dynamically mixed batches: it needs --dynamic_mix 1")
    if k < slots and loss == 'pit':
        raise SystemExit(f"--dm_min_speakers {k} with --C {args.C} leaves silent sources in the batch, and --loss pit "
                         f"scores a silent source as noise (SI-SNR against zero): use --loss pit_var")


def minibatch_rows(mb):
    """Rows of the batch that data.py cuts from one AudioDataset minibatch entry
    [utterances, *speakers, sample_rate, segment_len]: ceil(samples / segment_len) per utterance."""
    import math
    seg = mb[-1]
    return len(mb[0]) if seg < 0 else sum(math.ceil(int(u[1]) / seg) for u in mb[0])


def check_dm_speeds(args):
    """--dm_speeds needs --dynamic_mix 1 and percents the resampler supports."""
    from dynamic_mix import _speed_table
    if any(p != 100 for p in args.dm_speeds) and not args.dynamic_mix:
        raise ValueError("--dm_speeds perturbs the dynamically mixed sources: it needs --dynamic_mix 1")
    try:
        _speed_table(args.dm_speeds)
    except ValueError as e:
        raise ValueError(f"--dm_speeds: {e}") from None


def check_dm_aug(args):
    """--dm_rir_dir and --dm_noise_dir need --dynamic_mix 1; the ranges the library accepts."""
    import math
    from dynamic_mix import MAX_RIR_TAPS
    for flag in ("dm_rir_dir", "dm_noise_dir"):
        if getattr(args, flag) and not args.dynamic_mix:
            raise ValueError(f"--{flag} augments the dynamically mixed batches: it needs --dynamic_mix 1")
    if not 0.0 <= args.dm_rir_prob <= 1.0:
        raise ValueError(f"--dm_rir_prob {args.dm_rir_prob}: a probability in [0, 1]")
    if not 1 <= args.dm_rir_max_taps <= MAX_RIR_TAPS:
        raise ValueError(f"--dm_rir_max_taps {args.dm_rir_max_taps}: 1 to {MAX_RIR_TAPS}")
    if not all(math.isfinite(v) for v in args.dm_snr_db):
        raise ValueError(f"--dm_snr_db {args.dm_snr_db}: finite values")


def dynamic_mix_loader(args, static_loader, rank, world):
    """The training loader of --dynamic_mix 1 (cross validation keeps the fixed set)."""
    if not args.use_cuda:
        raise ValueError("--dynamic_mix 1 mixes on the GPU: it cannot be combined with --use_cuda 0")
    from dynamic_mix import DeviceCorpus, DynamicMixer, DynamicMixLoader, RirBank
    device = torch.device("cuda", torch.cuda.current_device())
    corpus = DeviceCorpus.from_json_dir(args.train_dir, args.sample_rate, device=device)
    rirs = noise = None
    if args.dm_rir_dir:
        rirs = RirBank.from_dir(args.dm_rir_dir, args.sample_rate, args.dm_rir_max_taps, device)
        if rank == 0:
            print("Dynamic mixing: {} room impulse responses, up to {} taps{}".format(
                len(rirs), rirs.max_len,
                "; {} truncated to {} taps".format(rirs.truncated, args.dm_rir_max_taps) if rirs.truncated else ""))
    if args.dm_noise_dir:
        noise = DeviceCorpus.from_wav_dir(args.dm_noise_dir, args.sample_rate, device)
        if rank == 0:
            print("Dynamic mixing: {} noise recordings ({:.1f} MB on the device)".format(noise.n_utts,
                                                                                       noise.nbytes / 1e6))
    # under MixIT --C counts the model's outputs, not the speakers of a single mixture
    speakers = args.mixit_speakers if getattr(args, 'loss', 'pit') == 'mixit' else args.C
    mixer = DynamicMixer(corpus, args.batch_size, speakers, int(args.segment * args.sample_rate), seed=args.dm_seed,
                         level_mode=args.dm_level_mode, level_db=tuple(args.dm_level_db), peak=args.dm_peak,
                         rank=rank, world=world, speeds=args.dm_speeds, rirs=rirs, rir_prob=args.dm_rir_prob,
                         noise=noise, snr_db=tuple(args.dm_snr_db),
                         min_speakers=getattr(args, 'dm_min_speakers', 0) or None)
    steps = args.dm_steps if args.dm_steps > 0 else len(static_loader)
    if rank == 0:
        print("Dynamic mixing: {} utterances ({:.1f} MB on the device), {} steps per epoch".format(
            corpus.n_utts, corpus.nbytes / 1e6, steps))
    return DynamicMixLoader(mixer, steps)


class Single(torch.nn.Module):
    """One-GPU stand-in for nn.DataParallel: exposes ``.module`` (solver.py:55)."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)


class FlatDP(Single):
    """One process per GPU: the gradients are averaged across ranks by one flat RCCL
    all-reduce after backward (ctn_dist.FlatGradAllReduce, run by the solver), which keeps
    the TemporalBlock gradient reductions deferred and batched; DistributedDataParallel's
    hooks need every gradient as it arrives (bench at world size 1: 2124 utt/s, DDP 1990, no exchange 2131)."""

    def __init__(self, module):
        super().__init__(module)
        import ctn_dist
        self.grad_sync = ctn_dist.FlatGradAllReduce(module.parameters())


def main(args):
    check_mixit(args)
    check_var(args)
    check_mixture_consistency(args)
    check_dm_speeds(args)
    check_dm_aug(args)
    if args.dynamic_mix and not args.use_cuda:
        raise ValueError("--dynamic_mix 1 mixes on the GPU: it cannot be combined with --use_cuda 0")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    # data
    tr_dataset = AudioDataset(args.train_dir, args.batch_size,
                              sample_rate=args.sample_rate, segment=args.segment)
    if args.loss == 'mixit':
        # a leftover minibatch of one utterance cannot form a mixture of mixtures; dropped here,
        # before the sampler shares the minibatches out, so every rank runs the same steps
        tr_dataset.minibatch = [mb for mb in tr_dataset.minibatch if minibatch_rows(mb) >= 2]
    cv_dataset = AudioDataset(args.valid_dir, batch_size=1,  # 1 -> use less GPU memory to do cv
                              sample_rate=args.sample_rate,
                              segment=-1, cv_maxlen=args.cv_maxlen)  # -1 -> use full audio
    tr_loader = AudioDataLoader(tr_dataset, batch_size=1,
                                sampler=MinibatchSampler(tr_dataset, rank, world, shuffle=args.shuffle),
                                num_workers=args.num_workers)
    cv_loader = AudioDataLoader(cv_dataset, batch_size=1,
                                sampler=MinibatchSampler(cv_dataset, rank, world, drop_last=False), num_workers=0)
    if args.dynamic_mix:
        tr_loader = dynamic_mix_loader(args, tr_loader, rank, world)
    data = {'tr_loader': tr_loader, 'cv_loader': cv_loader}
    # model
    model = ConvTasNet(args.N, args.L, args.B, args.H, args.P, args.X, args.R,
                       args.C, norm_type=args.norm_type, causal=args.causal,
                       mask_nonlinear=args.mask_nonlinear, mixture_consistency=getattr(args, 'mixture_consistency', 'none'))
    if args.bf16:
        model.act_dtype = torch.bfloat16
    if rank == 0:
        print(model)
    if args.use_cuda:
        model.cuda()
        if world == 1:
            model = Single(model)
        elif args.norm_type != 'BN':
            model = FlatDP(model)
        else:
            # BatchNorm: DDP also broadcasts rank 0's running statistics each forward.
            # Gradients as views into the RCCL buckets and a static graph: at world size 1
            # on one MI355X this took the DDP step from 21.8 to 18.8 ms (plain 18.3 ms)
            model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[local], gradient_as_bucket_view=True,
                                                              static_graph=True)
    else:
        model = Single(model)
    # optimizer
    if args.optimizer == 'sgd':
        optimizer = torch.optim.SGD(model.parameters(), lr=args.lr, momentum=args.momentum,
                                    weight_decay=args.l2)
    elif args.optimizer == 'adam':
        import ctn_optim
        optimizer = ctn_optim.Adam(model.parameters(), lr=args.lr, weight_decay=args.l2)
    else:
        print("Not support optimizer")
        return
    solver = Solver(data, model, optimizer, args)
    solver.train()
    if world > 1:
        dist.destroy_process_group()


if __name__ == '__main__':
    args = parser.parse_args()
    print(args)
    main(args)
