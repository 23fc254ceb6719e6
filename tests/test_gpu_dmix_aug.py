"""Reverberation and noise on the device (ctn_dmix_draw_aug / ctn_dmix_mix_aug through
dynamic_mix.py) against the numpy restatement: the drawn plans exactly, sources, mixture and
noise bit for bit given the read-back gains, the gains against fp64 arithmetic, the all-off and
all-dry paths against the plain entry points, invalid entries, the rank split, and training."""
import ctypes
import types

import numpy as np
import pytest
import torch

import dynamic_mix as dm

pytestmark = pytest.mark.gpu

# the corpus of test_gpu_dmix_speed.py: 12 utterances of 1..6000 samples, 3 speakers
LENS = [4200, 1000, 6000, 1, 3000, 1000, 2500, 4099, 999, 1200, 4500, 5100]
SPK = [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 2, 0]
AMP = [1.0, 0.2, 0.15, 1.0, 1.0, 0.2, 0.1, 1.0, 0.2, 1.0, 0.12, 0.15]
NLENS = [7, 2049, 6000, 4099, 4500]
NAMP = [0.5, 0.1, 0.05, 0.3, 0.2]
RIR_LENS = [1, 2, 257, 2048, 2049, 5000, 16384]
SLOW_FAST = (95, 100, 105)
TS = [7, 2049, 4099]
HALF_SEED = 11                                           # test_dmix_aug_cpu.py: dry and wet slots at rir_prob 0.5


def _waves(kind, lens, amps, seed):
    rng = np.random.default_rng(seed)
    out = []
    for n, a in zip(lens, amps):
        x = rng.uniform(-1.0, 1.0, n) * a
        x[[0, n // 3, n - 1]] = [a, -a, a]               # loud at both ends: every joint of the pool is non-silent
        out.append(np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) if kind == "int16"
                   else x.astype(np.float32))
    return out


def _rirs():
    rng = np.random.default_rng(7)
    out = []
    for n in RIR_LENS:
        h = 0.05 * rng.standard_normal(n) * np.exp(-np.arange(n) / 1500.0)
        h[-1] = -0.5                                     # loud first and last taps
        h[0] = 0.75 if n == 1 else 1.0
        out.append(h.astype(np.float32))
    return out


class Setup:
    def __init__(self, kind):
        self.corpus = dm.DeviceCorpus(_waves(kind, LENS, AMP, 0), SPK, "cuda")
        self.noise = dm.DeviceCorpus(_waves(kind, NLENS, NAMP, 1), list(range(len(NLENS))), "cuda")
        self.bank = dm.RirBank(_rirs(), "cuda")
        self.pool, self.npool = self.corpus.pool.cpu().numpy(), self.noise.pool.cpu().numpy()
        assert all(self.npool[o - 1] != 0 and self.npool[o] != 0 for o in self.noise.off_host[1:-1])
        rp = self.bank.pool.cpu().numpy()
        assert all(abs(rp[o - 1]) >= 0.5 and abs(rp[o]) >= 0.5 for o in self.bank.roff_host[1:-1])

    def mixer(self, M, C, T, rirs=True, noise=True, **kw):
        return dm.DynamicMixer(self.corpus, M, C, T, rirs=self.bank if rirs else None,
                               noise=self.noise if noise else None, **kw)


@pytest.fixture(scope="module", params=["int16", "fp32"])
def setup(request):
    return Setup(request.param)


@pytest.fixture(scope="module")
def setup16():
    return Setup("int16")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nplan(mx):
    return dm.plan_to_numpy(mx.nplan)[:, 0]


def _host_plan(s, mx, first):
    d, g = mx.desc, mx._aug
    return dm.plan_aug_host(s.corpus.off_host, s.corpus.spk_host, mx.elig_host, mx.M, mx.C, mx.T, seed=d.seed,
                            first_sample=first, level_db=(d.level_lo_db, d.level_hi_db), max_tries=d.max_tries,
                            speeds=mx.speeds, n_rirs=g.n_rirs, rir_prob=g.rir_prob,
                            noise_off=None if mx.noise is None else mx.noise.off_host, noise_elig=mx.nelig_host,
                            snr_db=(g.snr_lo_db, g.snr_hi_db))


def _assert_contract(s, mx, mixture, sources, noise_out=None, level_mode=0):
    """Sources, mixture and noise are the numpy contract applied to the read-back gains, bit for bit."""
    ref = dm.mix_aug_host(
        s.pool, s.corpus.off_host, dm.plan_to_numpy(mx.plan), mx.T, level_mode=level_mode, peak=mx.desc.peak,
        gains=mx.gains.cpu().numpy(), ngain=mx.ngain.cpu().numpy(), speeds=mx.speeds,
        speed_idx=None if mx.speeds is None else mx.speed.cpu().numpy(),
        rirs=None if mx.rirs is None else mx.rirs.rirs_host, rir=mx.rir.cpu().numpy(),
        noise_pool=None if mx.noise is None else s.npool, noise_off=None if mx.noise is None else mx.noise.off_host,
        nplan=None if mx.noise is None else _nplan(mx))
    assert np.array_equal(mx.status.cpu().numpy(), ref["status"])
    assert np.array_equal(_bits(sources.cpu().numpy()), _bits(ref["sources"]))
    assert np.array_equal(_bits(mixture.cpu().numpy()), _bits(ref["mixture"]))
    if noise_out is not None:
        assert np.array_equal(_bits(noise_out.cpu().numpy()), _bits(ref["noise"]))
    return ref


# ---------------------------------------------------------------------------- draw
@pytest.mark.parametrize("speeds", [None, SLOW_FAST])
@pytest.mark.parametrize("T", [7, 1000, 4099])
def test_draw_equals_host(setup16, T, speeds):
    s = setup16
    wet, dry, utts = 0, 0, set()
    for M, C in ((1, 1), (5, 2), (5, 3)):
        mx = s.mixer(M, C, T, seed=HALF_SEED, max_tries=8, speeds=speeds, rir_prob=0.5, snr_db=(-3.0, 7.0))
        assert mx.nelig_host.tolist() == [i for i, n in enumerate(NLENS) if n >= T]
        for first in (0, (1 << 40) + 5):
            dev = dm.plan_to_numpy(mx.draw(first))
            host = _host_plan(s, mx, first)
            nplan = _nplan(mx)
            for f in ("utt", "start", "tries"):
                assert np.array_equal(dev[f], host["plan"][f]), f
                assert np.array_equal(nplan[f], host["nplan"][f]), f
            for d, h in ((dev, host["plan"]), (nplan, host["nplan"])):
                assert (np.abs(d["level_db"] - h["level_db"]) <= np.spacing(np.abs(h["level_db"]))).all()
            if speeds is not None:
                assert np.array_equal(mx.speed.cpu().numpy(), host["speed_idx"])
            rir = mx.rir.cpu().numpy()
            assert rir.dtype == np.int32 and np.array_equal(rir, host["rir"])
            assert (nplan["start"] + T <= np.asarray(NLENS)[nplan["utt"]]).all()
            wet, dry = wet + int((rir >= 0).sum()), dry + int((rir < 0).sum())
            utts |= set(nplan["utt"].tolist())
    assert wet > 0 and dry > 0 and len(utts) > 1


def test_draw_device_counter(setup16):
    mx = setup16.mixer(5, 2, 1000, seed=4, speeds=SLOW_FAST, rir_prob=0.5)
    counter = torch.tensor([100], dtype=torch.int64, device="cuda")
    got = []
    for _ in range(2):
        plan = mx.draw(first_sample=-1, counter=counter, advance=5).clone()
        got.append((plan, mx.speed.clone(), mx.rir.clone(), mx.nplan.clone()))
    assert counter.item() == 110
    for want, first in zip(got, (100, 105)):
        mx.draw(first)
        for a, b in zip(want, (mx.plan, mx.speed, mx.rir, mx.nplan)):
            assert torch.equal(a, b)
    assert not torch.equal(got[0][2], got[1][2]) and not torch.equal(got[0][3], got[1][3])


# ---------------------------------------------------------------------------- contract, bit-exact
MODES = [(0, 0.9), (0, 0.0), (1, 0.9), (1, 0.0)]


@pytest.mark.parametrize("level_mode,peak", MODES)
@pytest.mark.parametrize("speeds", [None, SLOW_FAST])
@pytest.mark.parametrize("T", TS)
def test_mix_bit_exact_on_drawn_plan(setup, T, speeds, level_mode, peak):
    mx = setup.mixer(4, 2, T, seed=HALF_SEED, level_mode=level_mode, peak=peak, speeds=speeds, rir_prob=0.5)
    noise_out = torch.empty(4, T, device="cuda")
    seen = set()
    for step in (0, 1):                                  # the second call reuses the workspace
        mx.draw(mx.first_sample(step))
        mixture, sources = mx.mix(noise_out=noise_out)
        ref = _assert_contract(setup, mx, mixture, sources, noise_out, level_mode)
        assert not ref["status"].any() and sources.abs().amax(dim=2).min() > 0 and noise_out.abs().amax(dim=1).min() > 0
        seen |= set(mx.rir.cpu().numpy().ravel().tolist())
    assert -1 in seen and len(seen) > 2


def _hand_plan(T, speeds):
    """4 rows of C = 2: every RIR on some slot and one dry slot (row 3: wet and dry); sources at
    the starts 0, room, and interior ones; noise at 0, len - T, an odd and an even interior start."""
    need = T if speeds is None else max(dm.segment_span(T, *dm.speed_ratio(p)) for p in speeds)
    utts = [u for u in (2, 11, 10, 0, 7, 4) if LENS[u] >= need]
    plan, idx = [], []
    for i in range(8):
        u = utts[i % len(utts)]
        k = i % 3
        span = T if speeds is None else dm.segment_span(T, *dm.speed_ratio(speeds[k]))
        room = LENS[u] - span
        plan.append((u, [0, room, min(room, 1), min(room, 2), room // 2 | 1 if room else 0, room // 4 * 2][i % 6],
                     0.5 * (i % 7) - 1.5, 1))
        idx.append(k)
    nutts = [u for u, n in enumerate(NLENS) if n >= T]
    nplan = []
    for r in range(4):
        u = nutts[(r + 1) % len(nutts)] if r < 2 else max(nutts, key=lambda q: NLENS[q])
        room = NLENS[u] - T
        nplan.append((u, [0, room, min(room, (room // 2) | 1), room // 4 * 2][r], [-5.0, 0.0, 3.5, 12.0][r], 1))
    return (np.array(plan, dtype=dm.PLAN_DTYPE).reshape(4, 2), np.array(idx, np.int32).reshape(4, 2),
            np.array([0, 1, 2, 3, 4, 5, 6, -1], np.int32).reshape(4, 2), np.array(nplan, dtype=dm.PLAN_DTYPE))


WORST = {"gains": 0.0, "ngain": 0.0}


@pytest.mark.parametrize("level_mode,peak", MODES)
@pytest.mark.parametrize("speeds", [None, SLOW_FAST])
@pytest.mark.parametrize("T", TS)
def test_mix_hand_plans_guard_samples_and_gains(setup, T, speeds, level_mode, peak):
    plan, idx, rir, nplan = _hand_plan(T, speeds)
    M, C = plan.shape
    starts = nplan["start"].tolist()
    assert starts[0] == 0 and starts[1] == NLENS[nplan["utt"][1]] - T > 0 and starts[2] % 2 == 1 and starts[3] % 2 == 0
    if level_mode == 1 and peak > 0:
        peak = 3.0                                       # unit-RMS sources: 0.9 would scale every row
    mx = setup.mixer(M, C, T, level_mode=level_mode, peak=peak, speeds=speeds)
    # outputs inside larger buffers, at 12 and 20 bytes from their (aligned) beginnings
    gs, gm, mark = 3, 5, 12345.0
    sbuf = torch.full((gs + M * C * T + gs,), mark, device="cuda")
    mbuf = torch.full((gm + M * T + gm,), mark, device="cuda")
    nbuf = torch.full((gs + M * T + gs,), mark, device="cuda")
    sources, mixture = sbuf[gs:gs + M * C * T].view(M, C, T), mbuf[gm:gm + M * T].view(M, T)
    noise_out = nbuf[gs:gs + M * T].view(M, T)
    kw = dict(rir=torch.from_numpy(rir).cuda(), nplan=dm.plan_from_numpy(nplan.reshape(M, 1), "cuda"))
    if speeds is not None:
        kw["speed"] = torch.from_numpy(idx).cuda()
    mx.mix(dm.plan_from_numpy(plan, "cuda"), sources=sources, mixture=mixture, noise_out=noise_out, **kw)
    ref = _assert_contract(setup, mx, mixture, sources, noise_out, level_mode)
    assert not ref["status"].any()
    for buf, g in ((sbuf, gs), (mbuf, gm), (nbuf, gs)):
        assert (buf[:g] == mark).all() and (buf[-g:] == mark).all()
    # the gains against fp64 arithmetic: the source gains at the plain mix's 4 fp32 ulps, the noise
    # gain at 5 (one more rounding: it depends on the rounded source gains through P_s), on the
    # rows where one ulp of a gain cannot flip the guard's branch
    safe = np.abs(ref["p"] - peak) >= 1e-3 * peak if peak > 0 else np.ones(M, bool)
    assert safe.sum() >= M // 2
    for name, dev, want, ulps in (("gains", mx.gains, ref["gains"], 4.0), ("ngain", mx.ngain, ref["ngain"], 5.0)):
        got = dev.cpu().numpy()[safe].astype(np.float64)
        ulp = np.spacing(np.abs(want[safe]).astype(np.float32)).astype(np.float64)
        worst = float(np.max(np.abs(got - want[safe]) / ulp))
        WORST[name] = max(WORST[name], worst)
        print(f"{name}: worst {worst:.3f} ulp here, {WORST[name]:.3f} so far")
        assert worst <= ulps, name
    assert (mx.ngain.cpu().numpy() > 0).all()


# ---------------------------------------------------------------------------- off is off
def _aug_entry_points(s, mx, aug, rir, first, level_mode):
    """ctn_dmix_draw_aug + ctn_dmix_mix_aug themselves with the descriptor `aug`, on the buffers
    of a mixer that was built without rirs and noise -> (plan, gains, sources, mixture)."""
    import ctn_lib as L
    lib, c = L.load(), s.corpus
    plan, gains = torch.zeros_like(mx.plan), torch.full_like(mx.gains, 7.0)
    speed = None if mx.speed is None else torch.full_like(mx.speed, 7)
    sources = torch.empty(mx.M, mx.C, mx.T, device="cuda")
    mixture = torch.empty(mx.M, mx.T, device="cuda")
    status = torch.full_like(mx.status, 7)
    ws = L.workspace(lib.ctn_dmix_aug_workspace_bytes(ctypes.byref(mx.desc), mx._sp_ref(), ctypes.byref(aug)), "cuda")
    bank = s.bank if aug.n_rirs else None
    L.check(lib.ctn_dmix_draw_aug(ctypes.byref(mx.desc), mx._sp_ref(), ctypes.byref(aug), L.ptr(c.off), L.ptr(c.spk),
                                  L.ptr(mx.elig), None, None, first, None, 0, L.ptr(plan), L.ptr(speed), L.ptr(rir),
                                  None, L.stream_handle(c.device)), "ctn_dmix_draw_aug")
    L.check(lib.ctn_dmix_mix_aug(ctypes.byref(mx.desc), mx._sp_ref(), ctypes.byref(aug), L.ptr(mx._filt), L.ptr(c.pool),
                                 L.ptr(c.off), L.ptr(plan), L.ptr(speed), None if bank is None else L.ptr(bank.pool),
                                 None if bank is None else L.ptr(bank.roff), L.ptr(rir), None, None, None,
                                 L.ptr(gains), None, L.ptr(sources), L.ptr(mixture), None, L.ptr(status), L.ptr(ws),
                                 ws.numel(), L.stream_handle(c.device)), "ctn_dmix_mix_aug")
    assert not status.any()
    return plan, speed, gains, sources, mixture


@pytest.mark.parametrize("level_mode", [0, 1])
@pytest.mark.parametrize("speeds", [None, SLOW_FAST])
def test_off_is_off(setup, speeds, level_mode):
    import ctn_lib as L
    T = 2049
    plain = setup.mixer(6, 2, T, rirs=False, noise=False, seed=3, level_mode=level_mode,
                        peak=0.9 if level_mode == 0 else 3.0, speeds=speeds)
    assert plain._aug is None
    first = plain.first_sample(1)
    mix_p, _, src_p = plain.batch(1)
    assert not plain.status.any()
    want = (plain.plan, plain.speed, plain.gains, src_p, mix_p)
    rir = torch.full((6, 2), 5, dtype=torch.int32, device="cuda")
    got = _aug_entry_points(setup, plain, L.DmixAug(), rir, first, level_mode)
    assert (rir == -1).all()
    dry = _aug_entry_points(setup, plain, L.DmixAug(n_rirs=len(setup.bank), rir_max_taps=setup.bank.max_len, rir_prob=0.0),
                            rir, first, level_mode)
    assert (rir == -1).all()
    for other in (got, dry):
        for a, b in zip(want, other):
            assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
    # through the mixer: a bank that is never used
    mx = setup.mixer(6, 2, T, noise=False, seed=3, level_mode=level_mode, peak=plain.desc.peak, speeds=speeds,
                     rir_prob=0.0)
    mixture, _, sources = mx.batch(1)
    assert (mx.rir == -1).all() and torch.equal(mx.gains.view(torch.int32), plain.gains.view(torch.int32))
    assert torch.equal(sources.view(torch.int32), src_p.view(torch.int32))
    assert torch.equal(mixture.view(torch.int32), mix_p.view(torch.int32))


# ---------------------------------------------------------------------------- invalid entries
@pytest.mark.parametrize("speeds", [None, SLOW_FAST])
def test_invalid_entries_zero_their_rows(setup, speeds):
    T = 1000
    good = np.array([[(0, 1, 1.0, 1), (2, 6, -1.5, 1)], [(10, 3, 0.0, 1), (11, 2, 0.5, 1)]] * 3, dtype=dm.PLAN_DTYPE)
    idx = torch.from_numpy(np.array([[0, 2], [2, 1]] * 3, np.int32)).cuda()
    grir = np.array([[2, -1], [6, 3]] * 3, np.int32)
    gn = np.array([(2, 5, 1.0, 1), (4, 0, -2.0, 1)] * 3, dtype=dm.PLAN_DTYPE)
    brir, bn = grir.copy(), gn.copy()
    brir[1, 0] = -2
    brir[2, 1] = len(RIR_LENS)
    bn[3]["utt"] = -1
    bn[5] = (3, NLENS[3] - T + 1, 0.0, 1)                # start + T = len + 1; utterance 3 is not the last
    kw = {} if speeds is None else dict(speed=idx)
    outs = []
    for rir, nplan in ((brir, bn), (grir, gn)):
        mx = setup.mixer(6, 2, T, speeds=speeds)
        noise_out = torch.full((6, T), 5.0, device="cuda")
        mixture, sources = mx.mix(dm.plan_from_numpy(good, "cuda"), rir=torch.from_numpy(rir).cuda(),
                                  nplan=dm.plan_from_numpy(nplan.reshape(6, 1), "cuda"), noise_out=noise_out, **kw)
        _assert_contract(setup, mx, mixture, sources, noise_out)
        outs.append((mx, mixture, sources, noise_out))
    (mx, mixture, sources, noise_out), (ok, mixture_ok, sources_ok, noise_ok) = outs
    assert mx.status.cpu().tolist() == [0, 1, 1, 1, 0, 1] and not ok.status.any()
    for m in (1, 2, 3, 5):
        assert not sources[m].any() and not mixture[m].any() and not noise_out[m].any()
        assert not mx.gains[m].any() and mx.ngain[m] == 0
    for m in (0, 4):                                     # the valid rows do not feel their neighbours
        assert torch.equal(mixture[m], mixture_ok[m]) and torch.equal(sources[m], sources_ok[m])
        assert torch.equal(noise_out[m], noise_ok[m]) and sources[m].abs().amax(dim=1).min() > 0


def test_mixer_refuses_bad_tensors(setup16):
    mx = setup16.mixer(4, 2, 1000)
    plan = dm.plan_from_numpy(np.array([[(0, 0, 0.0, 1), (2, 0, 0.0, 1)]] * 4, dtype=dm.PLAN_DTYPE), "cuda")
    good = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    for rir in (good[:3], good.long(), good.cpu(), good.view(2, 4)):
        with pytest.raises(ValueError, match="rir"):
            mx.mix(plan, rir=rir)
    with pytest.raises(ValueError, match="nplan"):
        mx.mix(plan, nplan=torch.zeros(4, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="noise_out"):
        mx.mix(plan, noise_out=torch.zeros(4, 999, device="cuda"))
    with pytest.raises(ValueError, match="without rirs"):
        setup16.mixer(4, 2, 1000, rirs=False).mix(plan, rir=good)
    with pytest.raises(ValueError, match="without noise"):
        setup16.mixer(4, 2, 1000, noise=False).mix(plan, noise_out=torch.zeros(4, 1000, device="cuda"))
    import ctn_lib as L
    with pytest.raises(L.CtnLibraryError, match="rir_prob"):
        setup16.mixer(4, 2, 1000, rir_prob=1.5)
    with pytest.raises(ValueError, match="noise: no recording"):
        dm.DynamicMixer(setup16.corpus, 4, 2, 1000, noise=dm.DeviceCorpus([np.ones(999, np.int16)], [0], "cuda"))


# ---------------------------------------------------------------------------- split, repeat
def test_rank_split_invariance_and_repeatability(setup):
    kw = dict(C=2, T=1000, seed=HALF_SEED, level_mode=1, peak=2.0, speeds=SLOW_FAST, rir_prob=0.5)
    whole = setup.mixer(8, **kw)
    mix_w, _, src_w = whole.batch(3)
    parts = []
    for rank in (0, 1):
        mx = setup.mixer(4, rank=rank, world=2, **kw)
        mixture, _, sources = mx.batch(3)
        parts.append((mixture, sources, mx.gains, mx.ngain, mx.plan, mx.speed, mx.rir, mx.nplan))
    for i, w in enumerate((mix_w, src_w, whole.gains, whole.ngain, whole.plan, whole.speed, whole.rir, whole.nplan)):
        got = torch.cat([p[i] for p in parts])
        assert torch.equal(got.view(torch.int32), w.view(torch.int32)), i
    assert (whole.rir == -1).any() and (whole.rir >= 0).any()
    mix_2, _, src_2 = setup.mixer(8, **kw).batch(3)      # equal arguments, equal bits
    assert torch.equal(mix_2.view(torch.int32), mix_w.view(torch.int32))
    assert torch.equal(src_2.view(torch.int32), src_w.view(torch.int32))


# ---------------------------------------------------------------------------- end to end
def test_training_over_the_loader_with_rirs_and_noise(setup16, tmp_path):
    import conv_tasnet as ct
    import ctn_optim
    import solver as S
    import train

    def run():
        torch.manual_seed(0)
        model = train.Single(ct.ConvTasNet(64, 20, 64, 128, 3, 2, 2, 2).cuda())
        opt = ctn_optim.Adam(model.parameters(), lr=1e-3)
        mixer = setup16.mixer(3, 2, 4000, seed=9, speeds=SLOW_FAST, rir_prob=0.5)
        args = types.SimpleNamespace(use_cuda=1, epochs=1, half_lr=0, early_stop=0, max_norm=5.0,
                                     save_folder=str(tmp_path), checkpoint=0, continue_from="",
                                     model_path="final.pth.tar", print_freq=10, visdom=0, visdom_epoch=0, visdom_id="t")
        solver = S.Solver({"tr_loader": dm.DynamicMixLoader(mixer, 3), "cv_loader": None}, model, opt, args)
        mean = solver._run_one_epoch(0)
        assert not mixer.status.any() and (mixer.ngain > 0).all()
        return mean, [p.detach().clone() for p in model.parameters()]

    mean_a, params_a = run()
    mean_b, params_b = run()
    assert np.isfinite(mean_a) and mean_a == mean_b
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(params_a, params_b))
