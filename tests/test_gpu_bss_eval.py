"""Device BSS Eval (csrc/ctn_bss.hip, bss_eval.bss_criteria_device / bss_eval_sources_batch,
evaluate.cal_SDRi_batch, evaluate.py --sdr_device) against the host routine of bss_eval.py.

Signals: synthetic.speech_like references; estimate e = 0.9 s_e + 0.15 (sum of the other
references) + white noise at `noise` times the clean estimate's standard deviation, rounded
to fp32; every tensor is NaN beyond the utterance's length.  Expected values: the host
routine on trimmed fp64 copies.

Tolerance 1e-8 dB on every finite SDR / SIR / SAR: cond(G) * 2^-53 * (10 / ln 10), about
5e-10 dB at the cond(G) of about 1e6 of these inputs, times 20 for the summation order.  The
same algorithm (direct-form fp64 correlations, Cholesky) run on the CPU agreed with the host
routine within 4e-13 dB.

The mixture row (case 2, cal_SDRi_batch) is the fp32 sum of the references on the 16-bit grid
of a full-scale PCM_16 wav, which is what evaluate.py reads; its SAR is about 90 dB.  The
unquantised fp32 sum is checked too (test_case2_exact_sum_mixture): its SAR, about 152 dB,
measures the fp32 rounding of the sum through the cancellation ep - p_all, where the host
routine itself is up to 1.4e-8 dB away from an 80-bit evaluation of the same formulas (case 2,
utterance of 97 samples; the device algorithm in fp64 on the CPU: 3.1e-8 dB), so that entry
has a bound of its own, derived there.  GPU only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_DB = 1e-8
SR = 8000

#        C  flen  T     lengths           noise  shuffle
CASES = {
    1: (1, 16, 200, [200, 131, 64], 0.05, False),     # a length above flen by less than one tile
    2: (2, 16, 700, [700, 613, 97], 0.05, False),     # full [E = 3, C] matrix, mixture row included
    3: (3, 24, 611, [611, 400], 0.05, False),         # taps: no power of two, no multiple of 64
    4: (2, 64, 1500, [1500], 1e-3, False),            # SAR about 59 dB: cancellation
    5: (2, 512, 1100, [1100, 640], 0.05, False),      # the default filter, system order 1024
    6: (4, 32, 900, [900, 555], 0.05, True),          # estimates shuffled per utterance
}


def _signals(case):
    """-> refs [M, C, T], ests [M, C, T], mixture [M, T] fp32 CPU tensors (NaN padding), lengths."""
    import synthetic
    C, flen, T, lengths, noise, shuffle = CASES[case]
    M = len(lengths)
    rng = np.random.default_rng(100 + case)
    _, src = synthetic.speech_like(M, C, T, 7 * case)
    refs = src.numpy().astype(np.float64)
    mixing = 0.15 * np.ones((C, C)) + 0.75 * np.eye(C)
    clean = np.einsum("ec,mct->met", mixing, refs)
    ests = clean + noise * clean.std(axis=-1, keepdims=True) * rng.standard_normal(clean.shape)
    if shuffle:
        for m in range(M):
            ests[m] = ests[m][rng.permutation(C)]
    refs32, ests32 = refs.astype(np.float32), ests.astype(np.float32)
    mix32 = refs32.sum(axis=1)
    step = np.abs(mix32).max(axis=-1, keepdims=True) / 32767.0          # full-scale PCM_16
    mix32 = (np.round(mix32 / step) * step).astype(np.float32)
    for m, n in enumerate(lengths):
        refs32[m, :, n:] = np.nan
        ests32[m, :, n:] = np.nan
        mix32[m, n:] = np.nan
    return torch.from_numpy(refs32), torch.from_numpy(ests32), torch.from_numpy(mix32), lengths


_cache = {}


def _case(case):
    """Signals and the host routine's result per utterance, computed once per case."""
    import bss_eval
    if case not in _cache:
        refs, ests, mix, lengths = _signals(case)
        flen = CASES[case][1]
        host = [bss_eval.bss_eval_sources(refs[m, :, :n].double().numpy(), ests[m, :, :n].double().numpy(), flen=flen)
                for m, n in enumerate(lengths)]
        _cache[case] = (refs, ests, mix, lengths, flen, host)
    return _cache[case]


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin], err_msg=what)
    err = np.abs(got[fin] - want[fin]).max() if fin.any() else 0.0
    print(f"{what}: max |device - host| = {err:.3e} dB over {int(fin.sum())} values")
    assert err <= TOL_DB, what


def _batch(case):
    import bss_eval
    refs, ests, mix, lengths, flen, host = _case(case)
    got = bss_eval.bss_eval_sources_batch(refs.cuda(), ests.cuda(), torch.tensor(lengths), flen=flen)
    for k, name in enumerate(("sdr", "sir", "sar")):
        _close(got[k], np.stack([h[k] for h in host]), f"case {case} {name}")
    np.testing.assert_array_equal(got[3], np.stack([h[3] for h in host]))
    return got, host


def test_case1_single_reference():
    import bss_eval
    got, host = _batch(1)
    assert np.all(np.isposinf(got[1])) and np.all(np.isposinf(np.stack([h[1] for h in host])))
    np.testing.assert_array_equal(got[0], got[2])                  # SDR == SAR, as on the host
    np.testing.assert_array_equal(np.stack([h[0] for h in host]), np.stack([h[2] for h in host]))
    refs, ests, _, lengths, flen, _ = _case(1)
    status = bss_eval.bss_criteria_device(refs.cuda(), ests.cuda(), torch.tensor(lengths), flen)[3]
    assert status.tolist() == [0, 0, 0]


def test_case2_full_criteria_matrix():
    """Every (signal, reference) pair, the two estimates and the mixture."""
    import bss_eval
    refs, ests, mix, lengths, flen, _ = _case(2)
    sigs = torch.cat((ests, mix.unsqueeze(1)), dim=1)
    sdr, sir, sar, status = bss_eval.bss_criteria_device(refs.cuda(), sigs.cuda(), torch.tensor(lengths), flen)
    assert sdr.shape == (3, 3, 2) and sdr.dtype == torch.float64 and sdr.is_cuda
    assert status.tolist() == [0, 0, 0]
    want = np.empty((3, 3, 3, 2))
    for m, n in enumerate(lengths):
        r, s = refs[m, :, :n].double().numpy(), sigs[m, :, :n].double().numpy()
        for e in range(3):
            for j in range(2):
                want[:, m, e, j] = bss_eval._criteria(*bss_eval._decompose(r, s[e], j, flen))
    for k, (name, got) in enumerate((("sdr", sdr), ("sir", sir), ("sar", sar))):
        _close(got.cpu().numpy(), want[k], f"case 2 matrix {name}")
    _batch(2)


def test_case2_exact_sum_mixture():
    """The mixture as the unquantised fp32 sum of the references: e_artif is the rounding
    noise of that sum, SAR about 152 dB.  SDR and SIR keep the 1e-8 dB tolerance.  SAR =
    10 log10(|p_all|^2 / |ep - p_all|^2) cancels SAR / 20 decimal digits: each sample of p_all
    is a sum of C * flen fp64 products, so it carries about sqrt(C * flen) * 2^-53 * |p_all|
    of rounding; in the worst case (aligned with e_artif) that moves |e_artif|^2 by
    2 * sqrt(C * flen) * 2^-53 * 10^(SAR / 20) relative, i.e. (10 / ln 10) times that in dB,
    and device and host each carry it: the bound is twice that (5e-7 dB at 153 dB, C * flen
    = 32; a well-conditioned SAR of 26 dB would get 2e-13 dB from the same formula)."""
    import bss_eval
    refs, _, _, lengths, flen, _ = _case(2)
    mix = refs.sum(dim=1, keepdim=True)
    sdr, sir, sar, status = bss_eval.bss_criteria_device(refs.cuda(), mix.cuda(), torch.tensor(lengths), flen)
    assert status.tolist() == [0, 0, 0]
    want = np.empty((3, 3, 1, 2))
    for m, n in enumerate(lengths):
        r, s = refs[m, :, :n].double().numpy(), mix[m, 0, :n].double().numpy()
        for j in range(2):
            want[:, m, 0, j] = bss_eval._criteria(*bss_eval._decompose(r, s, j, flen))
    _close(sdr.cpu().numpy(), want[0], "exact-sum mixture sdr")
    _close(sir.cpu().numpy(), want[1], "exact-sum mixture sir")
    assert np.all(want[2] > 140.0)
    bound = 2 * (10 / np.log(10)) * 2 * np.sqrt(2 * flen) * 2.0 ** -53 * 10 ** (want[2] / 20)
    err = np.abs(sar.cpu().numpy() - want[2])
    print(f"exact-sum mixture sar: max |device - host| = {err.max():.3e} dB, bound {bound.min():.3e} dB")
    assert np.all(err <= bound)


@pytest.mark.parametrize("case", [3, 4, 5])
def test_cases_against_host(case):
    got, _ = _batch(case)
    if case == 4:
        assert np.all(got[2] > 50.0)                               # the low-noise case is what it claims


def test_case6_shuffled_estimates_recover_the_permutation():
    got, host = _batch(6)
    perms = np.stack([h[3] for h in host])
    assert any(list(p) != [0, 1, 2, 3] for p in perms)             # the shuffle moved something
    _, _, _, lengths, flen, _ = _case(6)
    import bss_eval
    refs, ests = _case(6)[0], _case(6)[1]
    fixed = bss_eval.bss_eval_sources_batch(refs.cuda(), ests.cuda(), torch.tensor(lengths),
                                            compute_permutation=False, flen=flen)
    np.testing.assert_array_equal(fixed[3], np.tile(np.arange(4), (2, 1)))
    m, n = 1, lengths[1]
    want = bss_eval.bss_eval_sources(refs[m, :, :n].double().numpy(), ests[m, :, :n].double().numpy(),
                                     compute_permutation=False, flen=flen)
    for k, name in enumerate(("sdr", "sir", "sar")):
        _close(fixed[k][m], want[k], f"case 6 unpermuted {name}")


def test_two_runs_are_bit_identical():
    import bss_eval
    refs, ests, mix, lengths, flen, _ = _case(2)
    r, s, n = refs.cuda(), torch.cat((ests, mix.unsqueeze(1)), dim=1).cuda(), torch.tensor(lengths)
    a = bss_eval.bss_criteria_device(r, s, n, flen)
    b = bss_eval.bss_criteria_device(r, s, n, flen)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_batch_is_split_under_the_workspace_limit(monkeypatch):
    """A workspace limit below two utterances' need: one call per utterance, same bits."""
    import bss_eval
    refs, ests, _, lengths, flen, _ = _case(2)
    r, s, n = refs.cuda(), ests.cuda(), torch.tensor(lengths)
    whole = bss_eval.bss_criteria_device(r, s, n, flen)
    import ctypes

    import ctn_lib as L
    one = L.load().ctn_bss_workspace_bytes(ctypes.byref(L.BssDesc(1, 2, 2, 700, flen)))
    monkeypatch.setattr(bss_eval, "WS_LIMIT", one + one // 2)
    for x, y in zip(whole, bss_eval.bss_criteria_device(r, s, n, flen)):
        assert torch.equal(x, y)


def test_fewer_samples_than_unknowns_goes_to_the_host():
    """lengths + flen - 1 < C * flen: the Gram matrix is rank-deficient by construction."""
    import bss_eval
    import synthetic
    _, src = synthetic.speech_like(1, 2, 64, 5)
    rng = np.random.default_rng(5)
    est = (src + 0.1 * torch.from_numpy(rng.standard_normal(src.shape)).float())
    refs, ests = src.clone(), est.clone()
    refs[:, :, 32:], ests[:, :, 32:] = float("nan"), float("nan")
    got = bss_eval.bss_eval_sources_batch(refs.cuda(), ests.cuda(), torch.tensor([32]), flen=32)
    want = bss_eval.bss_eval_sources(refs[0, :, :32].double().numpy(), ests[0, :, :32].double().numpy(), flen=32)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[0], w)                     # NaNs compare equal


def test_duplicate_reference_is_flagged_and_goes_to_the_host():
    import bss_eval
    import synthetic
    _, src = synthetic.speech_like(1, 2, 300, 9)
    src[0, 1] = src[0, 0]
    rng = np.random.default_rng(9)
    est = src + 0.1 * torch.from_numpy(rng.standard_normal(src.shape)).float()
    status = bss_eval.bss_criteria_device(src.cuda(), est.cuda(), None, 16)[3]
    assert status.tolist() == [1]
    got = bss_eval.bss_eval_sources_batch(src.cuda(), est.cuda(), flen=16)
    want = bss_eval.bss_eval_sources(src[0].double().numpy(), est[0].double().numpy(), flen=16)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g[0], w)


def test_batch_raises_the_host_errors():
    import bss_eval
    refs, ests, _, lengths, flen, _ = _case(2)
    with pytest.raises(ValueError, match="shape mismatch"):
        bss_eval.bss_eval_sources_batch(refs.cuda(), ests[:, :1].cuda(), torch.tensor(lengths), flen=flen)
    with pytest.raises(ValueError, match="shorter than"):
        bss_eval.bss_eval_sources_batch(refs.cuda(), ests.cuda(), torch.tensor([700, 613, 15]), flen=flen)
    zero = refs.clone()
    zero[1, 0, :613] = 0
    with pytest.raises(ValueError, match="all zeros"):
        bss_eval.bss_eval_sources_batch(zero.cuda(), ests.cuda(), torch.tensor(lengths), flen=flen)


def test_cal_sdri_batch_matches_cal_sdri():
    import evaluate
    refs, ests, mix, lengths, flen, _ = _case(5)
    got = evaluate.cal_SDRi_batch(refs.cuda(), ests.cuda(), mix.cuda(), torch.tensor(lengths))
    want = [evaluate.cal_SDRi(refs[m, :, :n].double().numpy(), ests[m, :, :n].double().numpy(),
                              mix[m, :n].double().numpy()) for m, n in enumerate(lengths)]
    _close(got, want, "cal_SDRi_batch")


def test_evaluator_sdr_device_matches_host(tmp_path):
    """evaluate.py --cal_sdr 1 with --sdr_device 0 and 1 on a tiny model and corpus."""
    import conv_tasnet as ct
    import evaluate
    import preprocess
    import synthetic
    from audio_io import write_wav
    root = str(tmp_path)
    for d in ("mix", "s1", "s2"):
        os.makedirs(os.path.join(root, "wav", "tt", d))
    for i, n in enumerate((1500, 1100)):
        mix, src = synthetic.speech_like(1, 2, n, 40 + i)
        scale = 0.3 / float(mix.abs().max())
        write_wav(os.path.join(root, "wav", "tt", "mix", f"u{i}.wav"), mix[0].numpy() * scale, SR)
        for c in range(2):
            write_wav(os.path.join(root, "wav", "tt", f"s{c + 1}", f"u{i}.wav"), src[0, c].numpy() * scale, SR)
    preprocess.preprocess_one_dir(os.path.join(root, "wav", "tt", "mix"), os.path.join(root, "json", "tt"), "mix", SR)
    for c in (1, 2):
        preprocess.preprocess_one_dir(os.path.join(root, "wav", "tt", f"s{c}"), os.path.join(root, "json", "tt"),
                                      f"s{c}", SR)
    torch.manual_seed(0)
    model = ct.ConvTasNet(64, 20, 64, 128, 3, 2, 2, 2)
    path = os.path.join(root, "model.pth.tar")
    torch.save(ct.ConvTasNet.serialize(model, torch.optim.Adam(model.parameters()), 1), path)
    records = []
    for dev in ("0", "1"):
        ev = evaluate.Evaluator(evaluate.parser.parse_args(
            ["--model_path", path, "--data_dir", os.path.join(root, "json", "tt"), "--batch_size", "2",
             "--num_workers", "0", "--cal_sdr", "1", "--sdr_device", dev]))
        ev.run()
        records.append(ev.records)
    assert len(records[0]) == len(records[1]) == 2
    assert [r[0] for r in records[0]] == [r[0] for r in records[1]]          # SI-SNRi untouched
    _close([r[1] for r in records[1]], [r[1] for r in records[0]], "Evaluator SDRi")
