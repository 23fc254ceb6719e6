"""Speed perturbation on the device (ctn_dmix_draw_sp / ctn_dmix_mix_sp through
dynamic_mix.py) against the numpy restatement: plan and speed indices exactly, the
resampled sources and the mixture bit for bit given the read-back gains, invalid entries,
the 1/1 path against the plain mix, the rank split, and a training epoch.

The corpus's longest utterance has 6000 samples, so at T = 4099 the 200 % entry of the
table (50, 200, 110) (a span of 8197 samples) fits nowhere: that table runs at T = 7 and
2049, the table (95, 100, 105) at every T."""
import ctypes
import types

import numpy as np
import pytest
import torch

import dynamic_mix as dm

pytestmark = pytest.mark.gpu

# 12 utterances of 1..6000 samples, 3 speakers; speaker 0 owns most, so that candidates are
# rejected.  Utterances 2, 10, 11 (all three speakers) hold the 4303 samples of T = 4099 at
# 105 %; utterance 7 (4099 samples) is 2 longer than the span of T = 2049 at 200 %.
LENS = [4200, 1000, 6000, 1, 3000, 1000, 2500, 4099, 999, 1200, 4500, 5100]
SPK = [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 2, 0]
AMP = [1.0, 0.2, 0.15, 1.0, 1.0, 0.2, 0.1, 1.0, 0.2, 1.0, 0.12, 0.15]
SLOW_FAST = (95, 100, 105)
WIDE = (50, 200, 110)


def _waves(kind):
    rng = np.random.default_rng(0)
    out = []
    for n, a in zip(LENS, AMP):
        x = rng.uniform(-1.0, 1.0, n) * a
        x[[0, n // 3, n - 1]] = [a, -a, a]               # loud at both ends: every joint of the pool is non-silent
        out.append(np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) if kind == "int16"
                   else x.astype(np.float32))
    return out


@pytest.fixture(scope="module", params=["int16", "fp32"])
def corpus(request):
    c = dm.DeviceCorpus(_waves(request.param), SPK, "cuda")
    pool = c.pool.cpu().numpy()
    assert all(pool[o - 1] != 0 and pool[o] != 0 for o in c.off_host[1:-1])
    return c


@pytest.fixture(scope="module")
def corpus16():
    return dm.DeviceCorpus(_waves("int16"), SPK, "cuda")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _spans(T, speeds):
    return [dm.segment_span(T, *dm.speed_ratio(p)) for p in speeds]


def _host_plan(c, mx, first):
    d = mx.desc
    return dm.plan_host(c.off_host, c.spk_host, mx.elig_host, mx.M, mx.C, mx.T, seed=d.seed, first_sample=first,
                        level_db=(d.level_lo_db, d.level_hi_db), max_tries=d.max_tries, speeds=mx.speeds)


def _assert_plan(dev, dev_speed, host):
    plan, idx = host
    for f in ("utt", "start", "tries"):
        assert np.array_equal(dev[f], plan[f]), f
    assert np.array_equal(dev_speed, idx) and dev_speed.dtype == np.int32
    assert (np.abs(dev["level_db"] - plan["level_db"]) <= np.spacing(np.abs(plan["level_db"]))).all()


def _assert_contract(c, mx, mixture, sources, level_mode=0):
    """Sources and mixture are the numpy contract applied to the read-back gains, bit for bit."""
    plan, gains = dm.plan_to_numpy(mx.plan), mx.gains.cpu().numpy()
    ref = dm.mix_host(c.pool.cpu().numpy(), c.off_host, plan, mx.T, level_mode=level_mode, peak=mx.desc.peak,
                      gains=gains, speeds=mx.speeds, speed_idx=mx.speed.cpu().numpy())
    assert np.array_equal(mx.status.cpu().numpy(), ref["status"])
    assert np.array_equal(_bits(sources.cpu().numpy()), _bits(ref["sources"]))
    assert np.array_equal(_bits(mixture.cpu().numpy()), _bits(ref["mixture"]))
    return ref


# ---------------------------------------------------------------------------- plan
@pytest.mark.parametrize("T", [7, 1000, 4099])
def test_plan_and_speed_equal_host(corpus16, T):
    rejected, seen = 0, set()
    for M in (1, 5):
        for C in (1, 2, 3):
            mx = dm.DynamicMixer(corpus16, M, C, T, seed=17 + C, max_tries=8, speeds=SLOW_FAST)
            assert mx.elig_host.tolist() == [i for i, n in enumerate(LENS) if n >= max(_spans(T, SLOW_FAST))]
            for first in (0, (1 << 40) + 5):
                dev, speed = dm.plan_to_numpy(mx.draw(first)), mx.speed.cpu().numpy()
                _assert_plan(dev, speed, _host_plan(corpus16, mx, first))
                n = np.diff(corpus16.off_host)[dev["utt"]]
                assert (dev["start"] + np.array(_spans(T, SLOW_FAST))[speed] <= n).all()
                rejected += int((dev["tries"] > 1).sum())
                seen |= set(speed.ravel().tolist())
    assert rejected > 0, "no candidate was ever rejected: the case does not test rejection"
    assert seen == {0, 1, 2}


def test_unit_table_gives_the_plain_plan(corpus16):
    """speeds (100,) are the plain entry points; the table {1/1} through ctn_dmix_draw_sp
    itself writes the plain plan's bits and speed 0 everywhere."""
    import ctn_lib as L
    plain = dm.DynamicMixer(corpus16, 5, 3, 1000, seed=4, max_tries=8)
    unit = dm.DynamicMixer(corpus16, 5, 3, 1000, seed=4, max_tries=8, speeds=(100,))
    assert unit.speed is None and unit.speeds is None
    for first in (0, (1 << 40) + 5):
        want = plain.draw(first).clone()
        assert torch.equal(unit.draw(first), want)
        table = L.DmixSpeeds(n=1)
        table.r[0].up = table.r[0].down = 1
        plan, speed = torch.zeros_like(want), torch.full((5, 3), 7, dtype=torch.int32, device="cuda")
        L.check(L.load().ctn_dmix_draw_sp(ctypes.byref(plain.desc), ctypes.byref(table), L.ptr(corpus16.off),
                                          L.ptr(corpus16.spk), L.ptr(plain.elig), first, None, 0, L.ptr(plan),
                                          L.ptr(speed), L.stream_handle(corpus16.device)), "ctn_dmix_draw_sp")
        assert torch.equal(plan, want) and not speed.any()


def test_plan_device_counter(corpus16):
    mx = dm.DynamicMixer(corpus16, 5, 2, 1000, seed=4, speeds=SLOW_FAST)
    counter = torch.tensor([100], dtype=torch.int64, device="cuda")
    got = []
    for _ in range(2):
        plan = dm.plan_to_numpy(mx.draw(first_sample=-1, counter=counter, advance=5))
        got.append((plan, mx.speed.cpu().numpy()))
    assert counter.item() == 110
    for (plan, speed), first in zip(got, (100, 105)):
        assert np.array_equal(dm.plan_to_numpy(mx.draw(first)), plan) and np.array_equal(mx.speed.cpu().numpy(), speed)
    assert not np.array_equal(got[0][0], got[1][0])


# ---------------------------------------------------------------------------- resampler, bit-exact
CASES = [(SLOW_FAST, 7), (SLOW_FAST, 2049), (SLOW_FAST, 4099), (WIDE, 7), (WIDE, 2049)]


@pytest.mark.parametrize("level_mode", [0, 1])
@pytest.mark.parametrize("speeds,T", CASES)
def test_mix_bit_exact_on_drawn_plan(corpus, speeds, T, level_mode):
    mx = dm.DynamicMixer(corpus, 5, 2, T, seed=23, level_mode=level_mode, speeds=speeds)
    seen = set()
    for step in (0, 1):                                  # the second call reuses workspace and outputs' slots
        mixture, _, sources = mx.batch(step)
        ref = _assert_contract(corpus, mx, mixture, sources, level_mode)
        assert not ref["status"].any() and sources.abs().amax(dim=2).min() > 0
        seen |= set(mx.speed.cpu().numpy().ravel().tolist())
    assert seen == {0, 1, 2}


def _hand_plan(T, speeds):
    """Rows of C = 2; every speed on every utterance that holds its span, at the starts 0,
    len - span, and an odd and an even interior sample.  -> (plan [M, 2], speed_idx [M, 2])"""
    slots = []
    for k, span in enumerate(_spans(T, speeds)):
        for u, n in enumerate(LENS):
            room = n - span
            if room < 0:
                continue
            for start in sorted({0, room, min(room, 1), min(room, 2), min(room, (room // 2) | 1), room // 4 * 2}):
                slots.append(((u, start, 0.5 * (len(slots) % 7) - 1.5, 1), k))
    if len(slots) % 2:
        slots.append(slots[0])
    order = np.random.default_rng(5).permutation(len(slots))
    plan = np.array([slots[i][0] for i in order], dtype=dm.PLAN_DTYPE).reshape(-1, 2)
    return plan, np.array([slots[i][1] for i in order], np.int32).reshape(-1, 2)


@pytest.mark.parametrize("level_mode", [0, 1])
@pytest.mark.parametrize("speeds,T", CASES)
def test_mix_hand_plans_and_guard_samples(corpus, speeds, T, level_mode):
    plan, idx = _hand_plan(T, speeds)
    M, C = plan.shape
    if (speeds, T) == (WIDE, 2049):                      # utterance 7: both filter tails overhang it
        tight = (plan["utt"] == 7) & (idx == 1)
        assert LENS[7] <= _spans(T, speeds)[1] + 3 and set(plan["start"][tight].tolist()) == {0, 1, 2}
    mx = dm.DynamicMixer(corpus, M, C, T, level_mode=level_mode, peak=0.9 if level_mode == 0 else 3.0, speeds=speeds)
    # outputs inside larger buffers, at 12 and 20 bytes from their (aligned) beginnings
    gs, gm, mark = 3, 5, 12345.0
    sbuf = torch.full((gs + M * C * T + gs,), mark, device="cuda")
    mbuf = torch.full((gm + M * T + gm,), mark, device="cuda")
    sources, mixture = sbuf[gs:gs + M * C * T].view(M, C, T), mbuf[gm:gm + M * T].view(M, T)
    mx.mix(dm.plan_from_numpy(plan, "cuda"), sources=sources, mixture=mixture,
           speed=torch.from_numpy(idx).cuda())
    ref = _assert_contract(corpus, mx, mixture, sources, level_mode)
    assert not ref["status"].any()
    for buf, g in ((sbuf, gs), (mbuf, gm)):
        assert (buf[:g] == mark).all() and (buf[-g:] == mark).all()
    # the gains against fp64 arithmetic on the same resampled segments, at the plain mix's
    # 4 fp32 ulps, on the rows where one ulp of a gain cannot flip the guard's branch
    peak = mx.desc.peak
    safe = np.abs(ref["p"] - peak) >= 1e-3 * peak
    assert safe.sum() >= M // 2
    dev = mx.gains.cpu().numpy()[safe].astype(np.float64)
    ulp = np.spacing(np.abs(ref["gains"][safe]).astype(np.float32)).astype(np.float64)
    assert (np.abs(dev - ref["gains"][safe]) <= 4.0 * ulp).all()
    again = dm.DynamicMixer(corpus, M, C, T, level_mode=level_mode, peak=peak, speeds=speeds)
    mixture2, sources2 = again.mix(dm.plan_from_numpy(plan, "cuda"), speed=torch.from_numpy(idx).cuda())
    assert torch.equal(mixture2.view(torch.int32), mixture.view(torch.int32))
    assert torch.equal(sources2.view(torch.int32), sources.view(torch.int32))


# ---------------------------------------------------------------------------- invalid entries
def test_invalid_entries_zero_their_rows(corpus):
    T = 1000
    spans = _spans(T, SLOW_FAST)
    good = np.array([[(0, 1, 1.0, 1), (2, 6, -1.5, 1)], [(10, 3, 0.0, 1), (11, 2, 0.5, 1)]] * 3,
                    dtype=dm.PLAN_DTYPE)
    gidx = np.array([[0, 2], [2, 1]] * 3, np.int32)
    bad, bidx = good.copy(), gidx.copy()
    bidx[1, 0] = -1
    bidx[2, 1] = len(SLOW_FAST)
    bad[4, 0] = (4, LENS[4] - spans[0] + 1, 0.0, 1)      # start + span = len + 1; utterance 4 is not the last
    extra = np.array([[(12, 0, 0.0, 1), (0, 0, 0.0, 1)], [(0, 0, 0.0, 1), (11, LENS[11] - spans[2] + 1, 0.0, 1)]],
                     dtype=dm.PLAN_DTYPE)                # utt == n_utts; past the end of the pool at 105 %
    bad, bidx = np.concatenate([bad, extra]), np.concatenate([bidx, np.array([[1, 1], [1, 2]], np.int32)])
    mx = dm.DynamicMixer(corpus, len(bad), 2, T, speeds=SLOW_FAST)
    mixture, sources = mx.mix(dm.plan_from_numpy(bad, "cuda"), speed=torch.from_numpy(bidx).cuda())
    assert mx.status.cpu().tolist() == [0, 1, 1, 0, 1, 0, 1, 1]
    _assert_contract(corpus, mx, mixture, sources)
    for m in (1, 2, 4, 6, 7):
        assert not sources[m].any() and not mixture[m].any() and not mx.gains[m].any()
    ok = dm.DynamicMixer(corpus, len(good), 2, T, speeds=SLOW_FAST)
    mixture_ok, sources_ok = ok.mix(dm.plan_from_numpy(good, "cuda"), speed=torch.from_numpy(gidx).cuda())
    assert not ok.status.any()
    for m in (0, 3, 5):                                  # the valid rows do not feel their neighbours
        assert torch.equal(mixture[m], mixture_ok[m]) and torch.equal(sources[m], sources_ok[m])
        assert sources[m].abs().amax(dim=1).min() > 0


def test_mixer_refuses_bad_speed_tensors_and_tables(corpus16):
    mx = dm.DynamicMixer(corpus16, 4, 2, 1000, speeds=SLOW_FAST)
    plan = dm.plan_from_numpy(np.array([[(0, 0, 0.0, 1), (2, 0, 0.0, 1)]] * 4, dtype=dm.PLAN_DTYPE), "cuda")
    good = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    for speed in (good[:3], good.long(), good.cpu(), good.view(2, 4)):
        with pytest.raises(ValueError, match="speed"):
            mx.mix(plan, speed=speed)
    with pytest.raises(ValueError, match="without speeds"):
        dm.DynamicMixer(corpus16, 4, 2, 1000).mix(plan, speed=good)
    with pytest.raises(ValueError, match="49"):
        dm.DynamicMixer(corpus16, 4, 2, 1000, speeds=(49, 100))
    with pytest.raises(ValueError, match="distinct speakers"):
        dm.DynamicMixer(corpus16, 4, 2, 4099, speeds=WIDE)          # no utterance holds 8197 samples


# ---------------------------------------------------------------------------- 1/1 slots, split, repeat
@pytest.mark.parametrize("level_mode", [0, 1])
def test_unit_slots_in_a_mixed_table_equal_the_plain_mix(corpus, level_mode):
    T = 2049
    plain = dm.DynamicMixer(corpus, 6, 2, T, seed=3, level_mode=level_mode, peak=0.9 if level_mode == 0 else 3.0)
    mix_p, _, src_p = plain.batch(1)
    mx = dm.DynamicMixer(corpus, 6, 2, T, level_mode=level_mode, peak=plain.desc.peak, speeds=SLOW_FAST)
    mixture, sources = mx.mix(plain.plan.clone(), speed=torch.ones(6, 2, dtype=torch.int32, device="cuda"))
    assert not mx.status.any() and not plain.status.any()
    assert torch.equal(mx.gains.view(torch.int32), plain.gains.view(torch.int32))
    assert torch.equal(sources.view(torch.int32), src_p.view(torch.int32))
    assert torch.equal(mixture.view(torch.int32), mix_p.view(torch.int32))


def test_rank_split_invariance_and_repeatability(corpus):
    kw = dict(C=2, T=1000, seed=31, level_mode=1, peak=2.0, speeds=SLOW_FAST)
    whole = dm.DynamicMixer(corpus, 8, **kw)
    mix_w, len_w, src_w = whole.batch(3)
    parts = []
    for rank in (0, 1):
        mx = dm.DynamicMixer(corpus, 4, rank=rank, world=2, **kw)
        mixture, lengths, sources = mx.batch(3)
        parts.append((mixture, sources, mx.gains.clone(), mx.plan.clone(), mx.speed.clone()))
    assert torch.equal(torch.cat([p[3] for p in parts]), whole.plan)
    assert torch.equal(torch.cat([p[4] for p in parts]), whole.speed) and len(whole.speed.unique()) > 1
    assert torch.equal(torch.cat([p[2] for p in parts]).view(torch.int32), whole.gains.view(torch.int32))
    assert torch.equal(torch.cat([p[1] for p in parts]).view(torch.int32), src_w.view(torch.int32))
    assert torch.equal(torch.cat([p[0] for p in parts]).view(torch.int32), mix_w.view(torch.int32))
    mix_2, _, src_2 = dm.DynamicMixer(corpus, 8, **kw).batch(3)     # equal arguments, equal bits
    assert torch.equal(mix_2.view(torch.int32), mix_w.view(torch.int32))
    assert torch.equal(src_2.view(torch.int32), src_w.view(torch.int32))


# ---------------------------------------------------------------------------- end to end
def test_training_epoch_over_the_loader_with_speeds(corpus16, tmp_path):
    import conv_tasnet as ct
    import ctn_optim
    import solver as S
    import train
    torch.manual_seed(0)
    model = train.Single(ct.ConvTasNet(64, 20, 64, 128, 3, 2, 2, 2).cuda())
    before = [p.detach().clone() for p in model.parameters()]
    opt = ctn_optim.Adam(model.parameters(), lr=1e-3)
    mixer = dm.DynamicMixer(corpus16, 3, 2, 4000, seed=9, speeds=SLOW_FAST)
    loader = dm.DynamicMixLoader(mixer, 3)
    args = types.SimpleNamespace(use_cuda=1, epochs=1, half_lr=0, early_stop=0, max_norm=5.0,
                                 save_folder=str(tmp_path), checkpoint=0, continue_from="",
                                 model_path="final.pth.tar", print_freq=10, visdom=0, visdom_epoch=0, visdom_id="t")
    mean = S.Solver({"tr_loader": loader, "cv_loader": None}, model, opt, args)._run_one_epoch(0)
    assert np.isfinite(mean)
    assert not mixer.status.any()
    assert all(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
