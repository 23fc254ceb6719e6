"""The dynamic mixer's speaker count on the device (ctn_dmix_thin through
DynamicMixer(min_speakers=...)) against dynamic_mix.thin_host: plan and count exactly, the batch
bit for bit from the host mix with the read-back gains on the plain, speed and reverberation +
noise paths, thinned sources exactly zero, the default untouched, one training step of a small
model with the PIT loss that knows silent sources, and train.py / evaluate.py end to end on a
corpus whose silent sources are all-zero files."""
import numpy as np
import pytest
import torch

import dynamic_mix as dm
from test_gpu_dmix_aug import AMP, LENS, NAMP, NLENS, SPK, _bits, _waves

pytestmark = pytest.mark.gpu

M, C, T = 64, 3, 2049                                    # two chunks of 2048 samples
SEED, FIRST = 20211, (1 << 33) + 7


@pytest.fixture(scope="module")
def corpus():
    return dm.DeviceCorpus(_waves("int16", LENS, AMP, 0), SPK, "cuda")


@pytest.fixture(scope="module")
def extras():
    rng = np.random.default_rng(3)
    rirs = []
    for _ in range(5):                                   # 64-tap responses
        h = 0.1 * rng.standard_normal(64) * np.exp(-np.arange(64) / 20.0)
        h[0] = 1.0
        rirs.append(h.astype(np.float32))
    return dm.RirBank(rirs, "cuda"), dm.DeviceCorpus(_waves("int16", NLENS, NAMP, 1), list(range(len(NLENS))), "cuda")


def _mixer(corpus, k, **kw):
    return dm.DynamicMixer(corpus, M, C, T, seed=SEED, min_speakers=k, **kw)


def _check_plan(mx, k, kw):
    """plan and count against thin_host: of the host's own plan (level_db of the kept slots to a
    spacing, as the draw tests compare it) and, byte for byte, of the device's un-thinned plan."""
    plain = _mixer(mx.corpus, None, **kw)
    base = dm.plan_to_numpy(plain.draw(FIRST)).copy()
    assert np.isfinite(base["level_db"]).all() and (plain.count.cpu().numpy() == C).all()
    dev, count = dm.plan_to_numpy(mx.draw(FIRST)), mx.count.cpu().numpy()
    want, wcount = dm.thin_host(base, M, C, SEED, FIRST, k)
    assert count.dtype == np.int32 and np.array_equal(count, wcount)
    assert dev.tobytes() == want.tobytes()
    assert sorted(set(count.tolist())) == list(range(k, C + 1))
    d = mx.desc
    host = dm.plan_host(mx.corpus.off_host, mx.corpus.spk_host, mx.elig_host, M, C, T, seed=SEED, first_sample=FIRST,
                        level_db=(d.level_lo_db, d.level_hi_db), max_tries=d.max_tries, speeds=mx.speeds)
    host = host if mx.speeds is None else host[0]
    hthin, hcount = dm.thin_host(host, M, C, SEED, FIRST, k)
    assert np.array_equal(count, hcount)
    for f in ("utt", "start", "tries"):
        assert np.array_equal(dev[f], hthin[f]), f
    kept = np.arange(C)[None, :] < count[:, None]
    assert np.isneginf(dev["level_db"][~kept]).all() and np.isneginf(hthin["level_db"][~kept]).all()
    assert (np.abs(dev["level_db"][kept] - hthin["level_db"][kept]) <= np.spacing(np.abs(hthin["level_db"][kept]))).all()
    return count, kept


def _check_batch(mx, count, kept, ref, mixture, sources, noise=None):
    """The host mix with the read-back gains, bit for bit; thinned slots exactly zero; the mixture
    is the fp32 sum of the kept sources (and the noise)."""
    src, mix = sources.cpu().numpy(), mixture.cpu().numpy()
    assert not mx.status.cpu().numpy().any() and not ref["status"].any()
    assert np.array_equal(_bits(src), _bits(ref["sources"])) and np.array_equal(_bits(mix), _bits(ref["mixture"]))
    gains = mx.gains.cpu().numpy()
    assert (gains[~kept] == 0).all() and (gains[kept] > 0).all()
    assert bool((sources.abs()[torch.from_numpy(~kept).cuda()] == 0).all())
    assert np.abs(src[kept]).max(-1).min() > 0
    for m in range(M):
        want = src[m, 0].copy()
        for c in range(1, int(count[m])):
            want = want + src[m, c]
        if noise is not None:
            want = want + noise[m]
        assert np.array_equal(mix[m], want), m
    assert np.allclose(gains[kept], ref["gains"][kept], rtol=1e-5)


@pytest.mark.parametrize("level_mode", [0, 1])
@pytest.mark.parametrize("k", [1, 2])
def test_plain_path(corpus, k, level_mode):
    kw = dict(level_mode=level_mode, level_db=(-2.5, 2.5) if level_mode == 0 else (-20.0, -15.0))
    mx = _mixer(corpus, k, **kw)
    count, kept = _check_plan(mx, k, kw)
    mixture, sources = mx.mix()
    ref = dm.mix_host(corpus.pool.cpu().numpy(), corpus.off_host, dm.plan_to_numpy(mx.plan), T,
                      level_mode=level_mode, peak=mx.desc.peak, gains=mx.gains.cpu().numpy())
    _check_batch(mx, count, kept, ref, mixture, sources)


@pytest.mark.parametrize("k", [1, 2])
def test_speed_path(corpus, k):
    kw = dict(speeds=(95, 100, 105))
    mx = _mixer(corpus, k, **kw)
    count, kept = _check_plan(mx, k, kw)
    mixture, sources = mx.mix()
    ref = dm.mix_host(corpus.pool.cpu().numpy(), corpus.off_host, dm.plan_to_numpy(mx.plan), T, peak=mx.desc.peak,
                      gains=mx.gains.cpu().numpy(), speeds=mx.speeds, speed_idx=mx.speed.cpu().numpy())
    _check_batch(mx, count, kept, ref, mixture, sources)


@pytest.mark.parametrize("k", [1, 2])
def test_noise_and_rir_path(corpus, extras, k):
    bank, noise = extras
    kw = dict(rirs=bank, noise=noise, rir_prob=0.7, snr_db=(0.0, 10.0))
    mx = _mixer(corpus, k, **kw)
    count, kept = _check_plan(mx, k, kw)
    nz = torch.empty(M, T, device="cuda")
    mixture, sources = mx.mix(noise_out=nz)
    ref = dm.mix_aug_host(corpus.pool.cpu().numpy(), corpus.off_host, dm.plan_to_numpy(mx.plan), T, peak=mx.desc.peak,
                          gains=mx.gains.cpu().numpy(), ngain=mx.ngain.cpu().numpy(), rirs=bank.rirs_host,
                          rir=mx.rir.cpu().numpy(), noise_pool=noise.pool.cpu().numpy(), noise_off=noise.off_host,
                          nplan=dm.plan_to_numpy(mx.nplan)[:, 0])
    assert np.array_equal(_bits(nz.cpu().numpy()), _bits(ref["noise"])) and (mx.ngain.cpu().numpy() > 0).all()
    _check_batch(mx, count, kept, ref, mixture, sources, noise=nz.cpu().numpy())
    assert np.allclose(mx.ngain.cpu().numpy(), ref["ngain"], rtol=1e-5)   # the noise power sees the kept sources only


def test_device_counter_and_rank_split(corpus):
    """The count follows the row's global sample: a device counter that the draw advances, and a
    batch split over two ranks, give the unsplit batch's plan and count."""
    whole = _mixer(corpus, 1)
    want, wcount = dm.plan_to_numpy(whole.draw(FIRST)).copy(), whole.count.cpu().numpy().copy()
    counter = torch.tensor([FIRST], dtype=torch.int64, device="cuda")
    mx = _mixer(corpus, 1)
    got = dm.plan_to_numpy(mx.draw(counter=counter, advance=M))
    assert got.tobytes() == want.tobytes() and np.array_equal(mx.count.cpu().numpy(), wcount)
    assert int(counter) == FIRST + M
    half = dm.DynamicMixer(corpus, M // 2, C, T, seed=SEED, min_speakers=1)
    for r in range(2):
        part = dm.plan_to_numpy(half.draw(FIRST + r * (M // 2)))
        sl = slice(r * (M // 2), (r + 1) * (M // 2))
        assert part.tobytes() == want[sl].tobytes() and np.array_equal(half.count.cpu().numpy(), wcount[sl])


@pytest.mark.parametrize("k", [None, C])
def test_default_is_todays_mixer(corpus, k):
    """min_speakers None or C: the plan and the batch of a mixer built without the argument."""
    old = dm.DynamicMixer(corpus, M, C, T, seed=SEED)
    new = _mixer(corpus, k)
    assert new.min_speakers is None
    a, b = dm.plan_to_numpy(old.draw(FIRST)), dm.plan_to_numpy(new.draw(FIRST))
    assert a.tobytes() == b.tobytes() and (new.count.cpu().numpy() == C).all()
    (m0, s0), (m1, s1) = old.mix(), new.mix()
    assert torch.equal(m0, m1) and torch.equal(s0, s1) and torch.equal(old.gains, new.gains)
    with pytest.raises(ValueError):
        _mixer(corpus, 0)
    with pytest.raises(ValueError):
        _mixer(corpus, C + 1)


def test_one_training_step_on_a_thinned_batch(corpus):
    """A small model separates a thinned batch into C outputs; cal_loss_var against the batch's
    sources (some all zero) with the batch's mixture, backward: a finite loss and a finite,
    non-zero gradient in every parameter."""
    import conv_tasnet as ct
    import pit_var_criterion as pv
    torch.manual_seed(0)
    mx = dm.DynamicMixer(corpus, 8, 3, 2000, seed=5, min_speakers=1)
    mixture, lengths, sources = mx.batch(0)
    assert mx.count.min() < 3
    model = ct.ConvTasNet(16, 20, 16, 16, 3, 2, 1, 3).cuda()
    est = model(mixture)
    loss, max_snr, perm, active = pv.cal_loss_var(sources, est, lengths, mixture)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(max_snr).all()
    assert torch.equal(active.sum(1).int(), mx.count)
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool(p.grad.abs().max() > 0), name


def _var_corpus(root):
    """tr/cv/tt splits of 3-speaker mixtures; in cv and tt some sources are all-zero files
    (cv u1: s3; tt u0: s3; tt u1: s2 and s3), the mixture the sum of the others."""
    import os

    import synthetic
    from audio_io import write_wav
    lengths = {"tr": [6400, 9000, 4500, 12000, 7000, 5000], "cv": [6000, 9500], "tt": [5000, 7300]}
    silent = {("cv", 1): (2,), ("tt", 0): (2,), ("tt", 1): (1, 2)}
    for split, lens in lengths.items():
        for d in ("mix", "s1", "s2", "s3"):
            os.makedirs(os.path.join(root, "wav", split, d), exist_ok=True)
        for i, n in enumerate(lens):
            _, src = synthetic.speech_like(1, 3, n, 17 * i + len(split))
            src = src[0] * (0.1 / float(src.abs().max()))
            for c in silent.get((split, i), ()):
                src[c] = 0.0
            write_wav(os.path.join(root, "wav", split, "mix", f"u{i}.wav"), src.sum(0).numpy(), 8000)
            for c in range(3):
                write_wav(os.path.join(root, "wav", split, f"s{c + 1}", f"u{i}.wav"), src[c].numpy(), 8000)


def test_train_and_evaluate_with_one_to_three_speakers(tmp_path, capsys):
    """train.py --dynamic_mix 1 --C 3 --dm_min_speakers 1 --loss pit_var end to end (mixture
    consistency on, validation on a fixed set with an all-zero source file), then evaluate.py
    --var_speakers 1 on a test set with silent sources: the three new figures are printed and
    ``records`` keeps its shape."""
    import os
    import types

    import evaluate
    import preprocess
    import train
    root = str(tmp_path)
    _var_corpus(root)
    preprocess.preprocess(types.SimpleNamespace(in_dir=os.path.join(root, "wav"), out_dir=os.path.join(root, "json"),
                                                sample_rate=8000))
    torch.manual_seed(0)
    train.main(train.parser.parse_args([
        "--train_dir", os.path.join(root, "json", "tr"), "--valid_dir", os.path.join(root, "json", "cv"),
        "--loss", "pit_var", "--dynamic_mix", "1", "--dm_min_speakers", "1", "--dm_steps", "3", "--C", "3",
        "--mixture_consistency", "uniform", "--N", "32", "--B", "32", "--H", "64", "--X", "2", "--R", "1",
        "--segment", "0.5", "--batch_size", "4", "--num_workers", "0", "--epochs", "2",
        "--save_folder", os.path.join(root, "exp"), "--print_freq", "1"]))
    pkg = torch.load(os.path.join(root, "exp", "final.pth.tar"), weights_only=True)
    assert np.isfinite(pkg["tr_loss"][:2].numpy()).all() and np.isfinite(pkg["cv_loss"][:2].numpy()).all()
    capsys.readouterr()
    ev = evaluate.Evaluator(evaluate.parser.parse_args([
        "--model_path", os.path.join(root, "exp", "final.pth.tar"), "--data_dir", os.path.join(root, "json", "tt"),
        "--batch_size", "2", "--num_workers", "0", "--var_speakers", "1"]))
    mean = ev.run()
    text = capsys.readouterr().out
    assert np.isfinite(mean) and len(ev.records) == 2 and all(len(r) == 2 and r[1] is None for r in ev.records)
    assert len(ev.var_records) == 2 and all(np.isfinite(r[0]) and isinstance(r[1], bool) for r in ev.var_records)
    for line in ("Average SISNR improvement over the active sources", "paired with silent sources",
                 "right number of outputs above -20 dB"):
        assert line in text, text
