"""Dynamic mixing on the device (ctn_dmix_draw / ctn_dmix_mix through dynamic_mix.py)
against its numpy restatement: the plan exactly, sources and mixture bit for bit under the
exactness contract, the gains within 4 fp32 ulps of fp64 arithmetic, invalid plan entries,
independence of the rank split, and a training epoch driven by the loader."""
import types

import numpy as np
import pytest
import torch

import dynamic_mix as dm

pytestmark = pytest.mark.gpu

# 12 utterances of 1..5000 samples, 3 speakers; speaker 0 owns most, so that candidates are
# rejected.  Utterances 0, 2, 7, 10, 11 (all three speakers) reach T = 4099; only 2 reaches 5000.
LENS = [4200, 1000, 5000, 1, 3000, 1000, 2500, 4099, 999, 1200, 4500, 4100]
SPK = [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 2, 0]
# amplitudes: full-scale utterances beside quiet ones, so that the peak guard takes both branches
AMP = [1.0, 0.2, 0.15, 1.0, 1.0, 0.2, 0.1, 1.0, 0.2, 1.0, 0.12, 0.15]


def _waves(kind):
    rng = np.random.default_rng(0)
    out = []
    for n, a in zip(LENS, AMP):
        x = rng.uniform(-1.0, 1.0, n) * a
        if n >= 1000:
            x[[0, n // 3, n - 1]] = [a, -a, a]           # the extremes, at the segment edges too
        out.append(np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) if kind == "int16"
                   else x.astype(np.float32))
    return out


@pytest.fixture(scope="module", params=["int16", "fp32"])
def corpus(request):
    return dm.DeviceCorpus(_waves(request.param), SPK, "cuda")


@pytest.fixture(scope="module")
def corpus16():
    return dm.DeviceCorpus(_waves("int16"), SPK, "cuda")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host_plan(c, mx, first):
    d = mx.desc
    return dm.plan_host(c.off_host, c.spk_host, mx.elig_host, mx.M, mx.C, mx.T, seed=d.seed, first_sample=first,
                        level_db=(d.level_lo_db, d.level_hi_db), max_tries=d.max_tries)


def _assert_plan(dev, host):
    for f in ("utt", "start", "tries"):
        assert np.array_equal(dev[f], host[f]), f
    assert (np.abs(dev["level_db"] - host["level_db"]) <= np.spacing(np.abs(host["level_db"]))).all()


def _assert_contract(c, mx, mixture, sources, level_mode=0):
    """Sources and mixture are the numpy contract applied to the read-back gains, bit for bit."""
    plan, gains = dm.plan_to_numpy(mx.plan), mx.gains.cpu().numpy()
    ref = dm.mix_host(c.pool.cpu().numpy(), c.off_host, plan, mx.T, level_mode=level_mode, peak=mx.desc.peak,
                      gains=gains)
    assert np.array_equal(mx.status.cpu().numpy(), ref["status"])
    assert np.array_equal(_bits(sources.cpu().numpy()), _bits(ref["sources"]))
    assert np.array_equal(_bits(mixture.cpu().numpy()), _bits(ref["mixture"]))
    return ref


# ---------------------------------------------------------------------------- plan
@pytest.mark.parametrize("T", [1, 7, 1000, 4099])
def test_plan_equals_host(corpus16, T):
    rejected = 0
    for M in (1, 5):
        for C in (1, 2, 3):
            mx = dm.DynamicMixer(corpus16, M, C, T, seed=17 + C, max_tries=8)
            for first in (0, 3 * M, (1 << 40) + 5):
                dev = dm.plan_to_numpy(mx.draw(first))
                _assert_plan(dev, _host_plan(corpus16, mx, first))
                rejected += int((dev["tries"] > 1).sum())
    assert rejected > 0, "no candidate was ever rejected: the case does not test rejection"


def test_plan_single_eligible_utterance(corpus16):
    mx = dm.DynamicMixer(corpus16, 5, 1, 5000, seed=1)
    assert mx.elig_host.tolist() == [2]
    dev = dm.plan_to_numpy(mx.draw(9))
    assert (dev["utt"] == 2).all() and (dev["start"] == 0).all() and (dev["tries"] == 1).all()
    _assert_plan(dev, _host_plan(corpus16, mx, 9))
    with pytest.raises(ValueError, match="distinct speakers"):
        dm.DynamicMixer(corpus16, 5, 2, 5000)


def test_plan_device_counter(corpus16):
    mx = dm.DynamicMixer(corpus16, 5, 2, 1000, seed=4)
    counter = torch.tensor([100], dtype=torch.int64, device="cuda")
    got = [dm.plan_to_numpy(mx.draw(first_sample=-1, counter=counter, advance=5)) for _ in range(2)]
    assert counter.item() == 110
    want = [dm.plan_to_numpy(mx.draw(first)) for first in (100, 105)]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not np.array_equal(got[0], got[1])


# ---------------------------------------------------------------------------- mix, bit-exact
@pytest.mark.parametrize("level_mode", [0, 1])
@pytest.mark.parametrize("T", [7, 1000, 4099])
def test_mix_bit_exact_on_drawn_plan(corpus, T, level_mode):
    mx = dm.DynamicMixer(corpus, 5, 2, T, seed=23, level_mode=level_mode)
    for step in (0, 1):                                  # the second call reuses workspace and outputs' slots
        mixture, _, sources = mx.batch(step)
        ref = _assert_contract(corpus, mx, mixture, sources, level_mode)
        assert not ref["status"].any()


def _hand_plan(T):
    """Rows of C = 2 whose starts are odd, even and len - T, on long utterances."""
    rows = []
    for a, b in ((0, 2), (2, 10), (7, 11), (10, 0), (11, 2)):
        rows.append([(a, min(1, LENS[a] - T), 1.0, 1), (b, LENS[b] - T, -1.5, 1)])
        rows.append([(a, LENS[a] - T, -2.5, 1), (b, 2 if LENS[b] - T >= 2 else 0, 2.5, 1)])
        rows.append([(a, min(3, LENS[a] - T), 0.0, 1), (b, min(6, LENS[b] - T), 0.25, 1)])
    return np.array(rows, dtype=dm.PLAN_DTYPE)


@pytest.mark.parametrize("T", [1000, 4099])
def test_mix_hand_plans_and_guard_samples(corpus, T):
    plan = _hand_plan(T)
    M, C = plan.shape
    mx = dm.DynamicMixer(corpus, M, C, T, peak=0.9)
    # outputs inside larger buffers, at 12 and 20 bytes from their (aligned) beginnings
    gs, gm, mark = 3, 5, 12345.0
    sbuf = torch.full((gs + M * C * T + gs,), mark, device="cuda")
    mbuf = torch.full((gm + M * T + gm,), mark, device="cuda")
    sources, mixture = sbuf[gs:gs + M * C * T].view(M, C, T), mbuf[gm:gm + M * T].view(M, T)
    mx.mix(dm.plan_from_numpy(plan, "cuda"), sources=sources, mixture=mixture)
    ref = _assert_contract(corpus, mx, mixture, sources)
    assert not ref["status"].any()
    for buf, g in ((sbuf, gs), (mbuf, gm)):
        assert (buf[:g] == mark).all() and (buf[-g:] == mark).all()


# ---------------------------------------------------------------------------- gains
def _ulps(dev, ref64):
    return np.abs(dev.astype(np.float64) - ref64) / np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("level_mode", [0, 1])
def test_gains_within_4_ulps_and_peak_guard(corpus, level_mode):
    """peak 0.9 (level_mode 0) / 3.0 (level_mode 1, unit-RMS sources): both branches occur.
    The 4 ulps: one each for the 10^x / RMS rounding, the dependence of p on the rounded
    gains, the division and the product.  Measured worst on an MI355X: 1.66 ulps."""
    peak = 0.9 if level_mode == 0 else 3.0
    mx = dm.DynamicMixer(corpus, 16, 2, 1000, seed=5, level_mode=level_mode, peak=peak)
    mixture, _, sources = mx.batch(2)
    ref = _assert_contract(corpus, mx, mixture, sources, level_mode)
    # a one-ulp gain difference must not be able to flip the guard's branch
    assert (np.abs(ref["p"] - peak) >= 1e-3 * peak).all(), ref["p"]
    guarded = ref["p"] > peak
    assert guarded.any() and (~guarded).any(), ref["p"]
    worst = _ulps(mx.gains.cpu().numpy(), ref["gains"]).max()
    print(f"level_mode {level_mode}: worst gain error {worst:.3f} fp32 ulps")
    assert worst <= 4.0
    assert np.abs(mixture.cpu().numpy()).max() <= peak * (1 + 1e-6)
    assert np.abs(mixture.cpu().numpy()[guarded]).max(axis=1).min() > peak * (1 - 1e-5)


def test_rms_mode_on_silence():
    c = dm.DeviceCorpus([np.zeros(300, np.int16), np.full(300, 1000, np.int16)], ["a", "b"], "cuda")
    mx = dm.DynamicMixer(c, 2, 2, 256, level_mode=1, peak=0.9)
    plan = np.array([[(0, 0, 2.0, 1), (0, 44, -1.0, 1)], [(0, 1, 0.0, 1), (1, 3, 0.0, 1)]], dtype=dm.PLAN_DTYPE)
    mixture, sources = mx.mix(dm.plan_from_numpy(plan, "cuda"))
    gains = mx.gains.cpu().numpy()
    assert np.isfinite(gains).all() and (gains > 0).all()
    assert not sources[0].any() and not mixture[0].any() and not sources[1, 0].any()
    assert mx.status.cpu().tolist() == [0, 0]
    _assert_contract(c, mx, mixture, sources, 1)
    assert _ulps(gains, dm.mix_host(c.pool.cpu().numpy(), c.off_host, plan, 256, 1, 0.9)["gains"]).max() <= 4.0


# ---------------------------------------------------------------------------- invalid entries
def test_invalid_plan_entry_zeroes_its_row(corpus):
    T = 1000
    good = _hand_plan(T)[:4]
    bad = good.copy()
    bad[1, 1] = (4, LENS[4] - T + 1, 0.0, 1)             # start + T = len + 1, utterance 4 is not the last
    bad[3, 0] = (12, 0, 0.0, 1)                          # utt == n_utts
    extra = np.array([[(-1, 0, 0.0, 1), (0, 0, 0.0, 1)], [(0, -1, 0.0, 1), (0, 0, 0.0, 1)]], dtype=dm.PLAN_DTYPE)
    bad = np.concatenate([bad, extra])
    mx = dm.DynamicMixer(corpus, len(bad), 2, T)
    mixture, sources = mx.mix(dm.plan_from_numpy(bad, "cuda"))
    assert mx.status.cpu().tolist() == [0, 1, 0, 1, 1, 1]
    ref = _assert_contract(corpus, mx, mixture, sources)
    for m in (1, 3, 4, 5):
        assert not sources[m].any() and not mixture[m].any() and not mx.gains[m].any()
    ok = dm.DynamicMixer(corpus, 4, 2, T)
    mixture_ok, sources_ok = ok.mix(dm.plan_from_numpy(good, "cuda"))
    for m in (0, 2):                                     # the valid rows do not feel their neighbours
        assert torch.equal(mixture[m], mixture_ok[m]) and torch.equal(sources[m], sources_ok[m])
    assert ref["status"].tolist() == [0, 1, 0, 1, 1, 1]


def test_mixer_refuses_tensors_the_library_would_overrun(corpus16):
    mx = dm.DynamicMixer(corpus16, 4, 2, 1000)
    good = dm.plan_from_numpy(_hand_plan(1000)[:4], "cuda")
    for plan in (good[:3], good.long(), good.cpu(), good.transpose(0, 1)):
        with pytest.raises(ValueError, match="plan"):
            mx.mix(plan)
    with pytest.raises(ValueError, match="sources"):
        mx.mix(good, sources=torch.empty(4, 2, 999, device="cuda"))
    with pytest.raises(ValueError, match="mixture"):
        mx.mix(good, mixture=torch.empty(4, 1000, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="counter"):
        mx.draw(counter=torch.zeros(1, dtype=torch.int32, device="cuda"))


# ---------------------------------------------------------------------------- split invariance
def test_rank_split_invariance(corpus):
    kw = dict(C=2, T=1000, seed=31, level_mode=1, peak=2.0)
    whole = dm.DynamicMixer(corpus, 8, **kw)
    mix_w, len_w, src_w = whole.batch(3)
    parts = []
    for rank in (0, 1):
        mx = dm.DynamicMixer(corpus, 4, rank=rank, world=2, **kw)
        mixture, lengths, sources = mx.batch(3)
        parts.append((mixture, sources, mx.gains.clone(), mx.plan.clone(), lengths))
    assert torch.equal(torch.cat([p[3] for p in parts]), whole.plan)
    assert torch.equal(torch.cat([p[2] for p in parts]).view(torch.int32), whole.gains.view(torch.int32))
    assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int32), src_w.view(torch.int32))
    assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int32), mix_w.view(torch.int32))
    assert torch.equal(torch.cat([p[4] for p in parts]), len_w) and len_w.dtype == torch.int64


# ---------------------------------------------------------------------------- end to end
def _train_epoch(corpus, tmp_path, monkeypatch):
    import conv_tasnet as ct
    import ctn_optim
    import solver as S
    import train
    torch.manual_seed(0)
    model = train.Single(ct.ConvTasNet(64, 20, 64, 128, 3, 2, 2, 2).cuda())
    before = [p.detach().clone() for p in model.parameters()]
    opt = ctn_optim.Adam(model.parameters(), lr=1e-3)
    loader = dm.DynamicMixLoader(dm.DynamicMixer(corpus, 3, 2, 4000, seed=9), 3)
    args = types.SimpleNamespace(use_cuda=1, epochs=1, half_lr=0, early_stop=0, max_norm=5.0,
                                 save_folder=str(tmp_path), checkpoint=0, continue_from="",
                                 model_path="final.pth.tar", print_freq=10, visdom=0, visdom_epoch=0, visdom_id="t")
    s = S.Solver({"tr_loader": loader, "cv_loader": None}, model, opt, args)
    losses, cal_loss = [], S.cal_loss

    def recording(*a, **k):
        out = cal_loss(*a, **k)
        losses.append(out[0].detach().clone())
        return out

    monkeypatch.setattr(S, "cal_loss", recording)
    mean = s._run_one_epoch(0)
    monkeypatch.setattr(S, "cal_loss", cal_loss)
    changed = [not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters())]
    return mean, torch.stack(losses).cpu(), changed


def test_training_epoch_over_the_loader(corpus16, tmp_path, monkeypatch):
    mean, losses, changed = _train_epoch(corpus16, tmp_path, monkeypatch)
    assert losses.shape == (3,) and torch.isfinite(losses).all() and np.isfinite(mean)
    assert all(changed)
    _, again, _ = _train_epoch(corpus16, tmp_path, monkeypatch)
    assert torch.equal(losses.view(torch.int32), again.view(torch.int32))
