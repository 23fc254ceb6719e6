#!/usr/bin/env python
"""Drop-in for ``src/evaluate.py``: SI-SNRi (and SDRi
when mir_eval is importable) of a trained model over a manifest directory.

Same flags and printout as the reference.  Differences, each deliberate:
* the forward runs on the HIP path (a ROCm device is required; the reference
  forces CUDA the same way, evaluate.py:44-46,57-61);
* SI-SNRi of all utterances of a minibatch is computed at once on the device
  in fp64 (``cal_SISNRi_batch``) for any number of speakers C (the reference
  loops over utterances in numpy and hard-codes C = 2, evaluate.py:73-84,117-124);
  ``cal_SISNR`` / ``cal_SISNRi`` keep the reference's numpy definitions
  (evaluate.py:108-144) and are what the batched version is tested against;
* ``--pit_fix 1`` pairs each target with the estimate its best permutation
  assigned to it; the reference's reorder_source uses the permutation itself,
  which mis-pairs 3-cycles for C >= 3 (pit_criterion.py:91-97).  Default 0 keeps
  the reference's pairing (identical for C = 2);
* SDRi uses mir_eval's bss_eval_sources (evaluate.py:10,90-105) when it is
  importable and otherwise ``bss_eval.bss_eval_sources``, a from-scratch
  restatement of the same BSS Eval v3 algorithm (mir_eval is not installed in
  this image, so SDRi parity is unpinned);
* ``--sdr_device 1`` (default 0: nothing changes) computes SDRi of a whole minibatch on
  the device with that restatement's algorithm (``cal_SDRi_batch``, csrc/ctn_bss.hip,
  DESIGN.md §18) instead of once per utterance on the host; same printout;
* ``--chunk_s SEC`` (default 0: nothing changes) separates every utterance in overlapping
  windows of SEC seconds stitched on the device (``longform.ChunkedSeparator``, DESIGN.md
  §23), so that the cost of windowing in SI-SNRi can be measured on a manifest;
* ``--cal_stoi 1`` (default 0: nothing changes) also scores STOI and ESTOI of a whole minibatch
  on the device (``cal_STOI_batch``, stoi.py, csrc/ctn_stoi.hip), for the
  paired estimates and for the unprocessed mixture; the reference has no such option;
* ``--mixit_remix 1`` (default 0: nothing changes) scores a MixIT-trained model, which has
  more outputs than the mixture has sources: its outputs are remixed to the two sources by
  the best assignment (``mixit_criterion.cal_mixit_loss``, csrc/ctn_mixit.hip)
  and the remixed pair takes the place of the PIT-paired estimates in every metric;
* ``--var_speakers 1`` (default 0: nothing changes) scores a model trained with ``--loss pit_var``
  on mixtures whose silent sources are all-zero files: outputs and sources are paired by
  ``pit_var_criterion.cal_loss_var`` (csrc/ctn_pitvar.hip), SI-SNRi is averaged
  over the active sources only, and ``var_records`` keeps, per utterance, the mean level of the
  outputs paired with silent sources (dB relative to the mixture) and whether the number of
  outputs above ``--var_count_db`` equals the number of active sources.
"""
import argparse

import numpy as np
import torch

from conv_tasnet import ConvTasNet
from data import AudioDataLoader, AudioDataset
from pit_criterion import cal_loss, cal_si_snr_with_pit
from utils import remove_pad

parser = argparse.ArgumentParser('Evaluate separation performance using Conv-TasNet')
parser.add_argument('--model_path', type=str, required=True,
                    help='Path to model file created by training')
parser.add_argument('--data_dir', type=str, required=True,
                    help='directory including mix.json, s1.json and s2.json')
parser.add_argument('--cal_sdr', type=int, default=0,
                    help='Whether calculate SDR, add this option because calculation of SDR is very slow')
parser.add_argument('--use_cuda', type=int, default=0,
                    help='Whether use GPU (the HIP path always runs on the GPU)')
parser.add_argument('--sample_rate', default=8000, type=int,
                    help='Sample rate')
parser.add_argument('--batch_size', default=1, type=int,
                    help='Batch size')
parser.add_argument('--num_workers', default=2, type=int,
                    help='DataLoader workers reading the wavs (the reference uses 2)')
parser.add_argument('--pit_fix', default=0, type=int,
                    help='1: pair targets with the inverse of the best permutation (C >= 3)')
parser.add_argument('--sdr_device', default=0, type=int,
                    help='1: with --cal_sdr 1, compute SDRi on the device (bss_eval, batched HIP kernels)')
parser.add_argument('--chunk_s', default=0.0, type=float,
                    help='Window in seconds for windowed separation (0: whole signal)')
parser.add_argument('--chunk_overlap_s', default=None, type=float,
                    help='Overlap of neighbouring windows in seconds (default: half of --chunk_s)')
parser.add_argument('--cal_stoi', default=0, type=int,
                    help='1: also compute STOI and ESTOI on the device (estimates and mixture, batched HIP kernels)')
parser.add_argument('--mixit_remix', default=0, type=int,
                    help='1: a MixIT-trained model with more outputs than sources: remix its outputs to the two '
                         'sources by the best assignment (batched HIP kernels) before they are scored')
parser.add_argument('--mixit_loss', default='snr', type=str, choices=['snr', 'si_snr'],
                    help='Score that picks the assignment of --mixit_remix 1')
parser.add_argument('--mixit_snr_max', default=30.0, type=float,
                    help='Soft SNR ceiling in dB of --mixit_loss snr')
parser.add_argument('--var_speakers', default=0, type=int,
                    help='1: the mixtures hold 1 to C speakers (silent sources are all-zero files): pair by the '
                         'pit_var loss, average SI-SNRi over the active sources, report the silent outputs')
parser.add_argument('--var_count_db', default=-20.0, type=float,
                    help='--var_speakers 1: an output above this level (dB relative to the mixture) counts as a speaker')
parser.add_argument('--var_loss', default='snr', type=str, choices=['snr', 'si_snr'],
                    help='Score of an active source that picks the pairing of --var_speakers 1')
parser.add_argument('--var_snr_max', default=30.0, type=float,
                    help='Soft SNR ceiling in dB of --var_loss snr')
parser.add_argument('--var_inactive_snr_max', default=20.0, type=float,
                    help='--var_speakers 1: ceiling in dB of a silent output\'s score')


def reorder_inverse(est, source, lengths):
    """Estimates reordered so that index c holds the estimate PIT assigned to target c."""
    _, perms, idx = cal_si_snr_with_pit(source, est.clone(), lengths)
    best = perms[idx]                                   # [B, C]: estimate i -> target best[b, i]
    inv = torch.empty_like(best)
    inv.scatter_(1, best, torch.arange(best.size(1), device=best.device).expand_as(best).contiguous())
    return torch.gather(est, 1, inv.unsqueeze(-1).expand(-1, -1, est.size(-1)))


class Evaluator:
    """Scores a trained model over one manifest directory (src/evaluate.py:33-90 behaviour:
    the same per-utterance printout and averages).  Minibatches are separated on the
    device, scored there in fp64 (SI-SNRi, cal_SISNRi_batch) and, with --cal_sdr, on the
    host (SDRi, cal_SDRi) or with --sdr_device on the device (cal_SDRi_batch); ``records``
    keeps one (SI-SNRi, SDRi or None) per utterance; with --cal_stoi, ``stoi_records`` keeps one
    (STOI, ESTOI, mixture STOI, mixture ESTOI) per utterance (cal_STOI_batch)."""

    def __init__(self, args):
        self.args = args
        if getattr(args, 'cal_stoi', 0):
            import stoi
            try:
                stoi.device_ratio(args.sample_rate)
            except ValueError as e:
                raise SystemExit(f"--cal_stoi 1: {e}")
        if getattr(args, 'var_speakers', 0) and (args.cal_sdr or getattr(args, 'cal_stoi', 0) or
                                                 getattr(args, 'mixit_remix', 0)):
            raise SystemExit("--var_speakers 1: BSS Eval and STOI are undefined against a silent source, and the "
                             "MixIT remix pairs differently: use it without --cal_sdr, --cal_stoi and --mixit_remix")
        self.model = ConvTasNet.load_model(args.model_path)
        print(self.model)
        self.model.eval().cuda()
        dataset = AudioDataset(args.data_dir, args.batch_size, sample_rate=args.sample_rate, segment=-1)
        self.loader = AudioDataLoader(dataset, batch_size=1, num_workers=args.num_workers)
        self.records = []
        self.stoi_records = []
        self.var_records = []
        from separate import make_chunker
        self.chunker = make_chunker(self.model, getattr(args, 'chunk_s', 0.0), getattr(args, 'chunk_overlap_s', None),
                                    args.sample_rate)

    def _forward(self, mixture, lengths):
        """[B, T] -> [B, C, T]: the whole-signal forward, or with --chunk_s each utterance
        windowed at its own length (zeros past it, as the padded forward's tail is ignored)."""
        if self.chunker is None:
            if getattr(self.model, 'mixture_consistency', 'none') != 'none':   # from the package
                return self.model(mixture, lengths)
            return self.model(mixture)
        from separate import chunked_estimates
        ests = chunked_estimates(self.chunker, mixture, lengths)
        out = mixture.new_zeros((mixture.size(0), ests[0].size(0), mixture.size(1)))
        for b, e in enumerate(ests):
            out[b, :, :e.size(1)] = e
        return out

    def _separate(self, mixture, lengths, source):
        """-> estimates paired with the targets (the reference's reorder, or --pit_fix)."""
        est = self._forward(mixture, lengths)                       # [B, C, T]
        if getattr(self.args, 'mixit_remix', 0):
            # a MixIT model has more outputs than sources: remix[b, n] is the sum of the outputs
            # that the best assignment gives to source n, already paired with it
            from mixit_criterion import cal_mixit_loss
            if source.size(1) != 2:
                raise ValueError("--mixit_remix 1 remixes to two sources per mixture, got %d" % source.size(1))
            return cal_mixit_loss(source, est.contiguous(), lengths, getattr(self.args, 'mixit_loss', 'snr'),
                                  getattr(self.args, 'mixit_snr_max', 30.0))[3]
        if getattr(self.args, 'var_speakers', 0):
            from pit_var_criterion import cal_loss_var
            est = est.contiguous()
            _, _, perm, active = cal_loss_var(source, est, lengths, mixture, getattr(self.args, 'var_loss', 'snr'),
                                              getattr(self.args, 'var_snr_max', 30.0),
                                              getattr(self.args, 'var_inactive_snr_max', 20.0))
            self._var = cal_var_batch(source, est, mixture, lengths, perm, active,
                                      getattr(self.args, 'var_count_db', -20.0))
            return pair_by_perm(est, perm)
        _, _, est, paired = cal_loss(source, est, lengths)
        if self.args.pit_fix:
            paired = reorder_inverse(est, source, lengths)
        return paired

    def _score(self, mixture, lengths, source, paired):
        if getattr(self.args, 'var_speakers', 0):
            return [(si, None) for si in self._var[0].cpu().tolist()]
        sisnri = cal_SISNRi_batch(source, paired, mixture, lengths).cpu().tolist()
        sdri = [None] * len(sisnri)
        if self.args.cal_sdr and getattr(self.args, 'sdr_device', 0):
            sdri = cal_SDRi_batch(source, paired, mixture, lengths).tolist()
        elif self.args.cal_sdr:
            mix_u, src_u, est_u = (remove_pad(t, lengths) for t in (mixture, source, paired))
            sdri = [cal_SDRi(src_u[b], est_u[b], mix_u[b]) for b in range(len(sisnri))]
        return list(zip(sisnri, sdri))

    @torch.no_grad()
    def run(self):
        for mixture, lengths, source in self.loader:
            mixture, lengths, source = mixture.cuda(), lengths.cuda(), source.cuda()
            paired = self._separate(mixture, lengths, source)
            st = [None] * mixture.size(0)
            if getattr(self.args, 'cal_stoi', 0):
                st = list(zip(*(v.tolist() for v in cal_STOI_batch(source, paired, mixture, lengths,
                                                                    self.args.sample_rate))))
            for (si, sd), sv in zip(self._score(mixture, lengths, source, paired), st):
                self.records.append((si, sd))
                print("Utt", len(self.records))
                if sd is not None:
                    print("\tSDRi={0:.2f}".format(sd))
                print("\tSI-SNRi={0:.2f}".format(si))
                if sv is not None:
                    self.stoi_records.append(sv)
                    print("\tSTOI={0:.3f}".format(sv[0]))
                    print("\tESTOI={0:.3f}".format(sv[1]))
            if getattr(self.args, 'var_speakers', 0):
                _, silent_db, count_ok = (v.cpu().tolist() for v in self._var)
                self.var_records.extend(zip(silent_db, count_ok))
        if self.var_records:
            return self._var_summary()
        n = len(self.records)
        if self.args.cal_sdr:
            print("Average SDR improvement: {0:.2f}".format(sum(r[1] for r in self.records) / n))
        mean_sisnri = sum(r[0] for r in self.records) / n
        print("Average SISNR improvement: {0:.2f}".format(mean_sisnri))
        if self.stoi_records:
            for k, name in enumerate(("STOI", "ESTOI", "STOI of the mixture", "ESTOI of the mixture")):
                print("Average {0}: {1:.3f}".format(name, sum(r[k] for r in self.stoi_records) / n))
        return mean_sisnri


    def _var_summary(self):
        """The averages of --var_speakers 1 (NaN: no utterance has such a source)."""
        si = [r[0] for r in self.records if r[0] == r[0]]
        quiet = [r[0] for r in self.var_records if r[0] == r[0]]
        mean_sisnri = sum(si) / len(si) if si else float("nan")
        print("Average SISNR improvement over the active sources: {0:.2f}".format(mean_sisnri))
        print("Average level of the outputs paired with silent sources: {0:.1f} dB relative to the mixture"
              .format(sum(quiet) / len(quiet) if quiet else float("nan")))
        print("Utterances with the right number of outputs above {0:.0f} dB: {1:.1f} %".format(
            getattr(self.args, 'var_count_db', -20.0),
            100.0 * sum(1 for r in self.var_records if r[1]) / len(self.var_records)))
        return mean_sisnri


def pair_by_perm(est, perm):
    """est [B, C, T], perm [B, C] (perm[b, i] = the source of output i) -> the outputs in source
    order: index j holds the output paired with source j."""
    inv = torch.empty_like(perm)
    inv.scatter_(1, perm, torch.arange(perm.size(1), device=perm.device).expand_as(perm).contiguous())
    return torch.gather(est, 1, inv.unsqueeze(-1).expand(-1, -1, est.size(-1)))


def cal_var_batch(source, est, mixture, lengths, perm, active, count_db=-20.0, eps=1e-8):
    """The figures of --var_speakers 1 for a padded batch (fp64, on the tensors' device): source /
    est [B, C, T], mixture [B, T], lengths [B], perm / active [B, C] from cal_loss_var ->
    (SI-SNRi [B] averaged over the active sources, level [B] in dB relative to the mixture averaged
    over the outputs paired with silent sources, count_ok [B] bool: as many outputs above
    count_db as active sources).  NaN where an utterance has no such source."""
    B, C, T = source.shape
    dev = source.device
    lengths = lengths.to(dev)
    valid = (torch.arange(T, device=dev).unsqueeze(0) < lengths.unsqueeze(1)).double()          # [B, T]
    mask, n = valid.unsqueeze(1).expand(B, C, T), lengths.double().unsqueeze(1).expand(B, C)
    s, e, x = source.double(), pair_by_perm(est, perm).double(), mixture.double()
    gain = _sisnr_rows(s, e, mask, n, eps) - _sisnr_rows(s, x.unsqueeze(1).expand(B, C, T), mask, n, eps)
    act = active.to(dev).double()
    nan = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    k = act.sum(1)
    sisnri = torch.where(k > 0, (gain * act).sum(1) / k.clamp(min=1), nan)
    level = 10 * torch.log10(((e * e * mask).sum(-1) + eps) / ((x * x * valid).sum(-1, keepdim=True) + eps))   # [B, C]
    silent_db = torch.where(k < C, (level * (1 - act)).sum(1) / (C - k).clamp(min=1), nan)
    count_ok = (level > count_db).sum(1) == active.to(dev).sum(1)
    return sisnri, silent_db, count_ok


def evaluate(args):
    """src/evaluate.py:33's entry point: score the model, return the mean SI-SNRi."""
    return Evaluator(args).run()


def cal_SDRi(src_ref, src_est, mix):
    """evaluate.py:90-105 (C speakers): mean over sources of SDR(est) - SDR(mixture)."""
    try:
        from mir_eval.separation import bss_eval_sources
    except ImportError:          # this image: the from-scratch BSS Eval v3 (parity unpinned)
        from bss_eval import bss_eval_sources
    src_anchor = np.stack([mix] * src_ref.shape[0], axis=0)
    sdr, sir, sar, popt = bss_eval_sources(src_ref, src_est)
    sdr0, sir0, sar0, popt0 = bss_eval_sources(src_ref, src_anchor)
    return float(np.mean(sdr - sdr0))


def cal_SDRi_batch(source, estimate, mixture, lengths, flen=None):
    """cal_SDRi of every utterance of a padded batch with bss_eval's device path: source /
    estimate [B, C, T], mixture [B, T], lengths [B] -> numpy [B].  One library call scores
    E = C + 1 signals per utterance, the C estimates and the mixture (the anchor's SDR
    against reference j is the same for every permutation of C copies of the mixture)."""
    import bss_eval
    flen = bss_eval.FLEN if flen is None else flen
    lengths, n = bss_eval._check_batch(source, estimate, lengths, flen)
    B, C, T = source.shape
    sigs = torch.cat((estimate, mixture.reshape(B, 1, T).to(estimate.dtype)), dim=1)
    sdr, sir, sar, status = (t.cpu().numpy() for t in bss_eval.bss_criteria_device(source, sigs, lengths, flen))
    out = np.empty(B)
    for b, host in enumerate(bss_eval._on_host(status, n, C, flen)):
        if host:
            src_u, est_u = (t[b, :, :n[b]].double().cpu().numpy() for t in (source, estimate))
            anchor = np.stack([mixture[b, :n[b]].double().cpu().numpy()] * C, axis=0)
            out[b] = np.mean(bss_eval.bss_eval_sources(src_u, est_u, flen=flen)[0] -
                             bss_eval.bss_eval_sources(src_u, anchor, flen=flen)[0])
        else:
            out[b] = np.mean(bss_eval._assign(sdr[b, :C], sir[b, :C], sar[b, :C], True)[0] - sdr[b, C])
    return out


def cal_STOI_batch(source, estimate, mixture, lengths, fs=8000):
    """STOI and ESTOI of every utterance of a padded batch with stoi.py's device path: source /
    estimate [B, C, T] (estimate c paired with source c), mixture [B, T], lengths [B] ->
    four numpy [B]: STOI and ESTOI of the estimates, STOI and ESTOI of the mixture against
    each source, each the mean over the sources.  One library call scores E = C + 1 signals
    per utterance, the C estimates and the mixture."""
    import stoi
    if source.dim() != 3 or source.shape != estimate.shape:
        raise ValueError(f"shape mismatch: sources {tuple(source.shape)}, estimates {tuple(estimate.shape)}")
    B, C, T = source.shape
    sigs = torch.cat((estimate, mixture.reshape(B, 1, T).to(estimate.dtype)), dim=1)
    d, de, _, _ = stoi.stoi_device(source, sigs, lengths, fs)                 # [B, C + 1, C]
    own = torch.arange(C, device=d.device)
    out = (d[:, own, own].mean(1), de[:, own, own].mean(1), d[:, C, :].mean(1), de[:, C, :].mean(1))
    return tuple(v.cpu().numpy() for v in out)


def cal_SISNRi(src_ref, src_est, mix):
    """evaluate.py:108-125 for C speakers: mean over c of SI-SNR(ref_c, est_c) - SI-SNR(ref_c, mix)
    (for C = 2 the same operations in the same order as the reference)."""
    acc = 0.0
    for c in range(src_ref.shape[0]):
        acc = acc + (cal_SISNR(src_ref[c], src_est[c]) - cal_SISNR(src_ref[c], mix))
    return acc / src_ref.shape[0]


def cal_SISNR(ref_sig, out_sig, eps=1e-8):
    """evaluate.py:128-144: scale-invariant SNR in dB of one signal pair (numpy)."""
    assert len(ref_sig) == len(out_sig)
    ref_sig = ref_sig - np.mean(ref_sig)
    out_sig = out_sig - np.mean(out_sig)
    ref_energy = np.sum(ref_sig ** 2) + eps
    proj = np.sum(ref_sig * out_sig) * ref_sig / ref_energy
    noise = out_sig - proj
    ratio = np.sum(proj ** 2) / (np.sum(noise ** 2) + eps)
    return 10 * np.log(ratio + eps) / np.log(10.0)


def _sisnr_rows(ref, out, mask, n, eps):
    """cal_SISNR over the last dim of fp64 tensors, restricted to mask (n valid samples)."""
    ref = (ref - (ref * mask).sum(-1, keepdim=True) / n.unsqueeze(-1)) * mask
    out = (out - (out * mask).sum(-1, keepdim=True) / n.unsqueeze(-1)) * mask
    ref_energy = (ref * ref).sum(-1, keepdim=True) + eps
    proj = (ref * out).sum(-1, keepdim=True) * ref / ref_energy
    noise = out - proj
    ratio = (proj * proj).sum(-1) / ((noise * noise).sum(-1) + eps)
    return 10 * torch.log(ratio + eps) / np.log(10.0)


def cal_SISNRi_batch(source, estimate, mixture, lengths, eps=1e-8):
    """SI-SNRi of every utterance of a padded batch at once (fp64, on the tensors' device):
    source/estimate [B, C, T], mixture [B, T], lengths [B] -> [B]; utterance b uses its first
    lengths[b] samples, as cal_SISNRi on remove_pad output (evaluate.py:67-84)."""
    B, C, T = source.shape
    dev = source.device
    lengths = lengths.to(dev)
    mask = (torch.arange(T, device=dev).unsqueeze(0) < lengths.unsqueeze(1)).double().unsqueeze(1).expand(B, C, T)
    n = lengths.double().unsqueeze(1).expand(B, C)
    s, e = source.double(), estimate.double()
    m = mixture.double().unsqueeze(1).expand(B, C, T)
    return (_sisnr_rows(s, e, mask, n, eps) - _sisnr_rows(s, m, mask, n, eps)).mean(1)


if __name__ == '__main__':
    args = parser.parse_args()
    print(args)
    evaluate(args)
