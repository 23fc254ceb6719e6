"""Reverberation and noise of dynamic mixing (dynamic_mix.py; ctn_dmix_draw_aug /
ctn_dmix_mix_aug) checks that need no GPU: the host convolution against numpy.convolve, the
properties of the host plan, the noise level and the pool joints of the host mix, the C
entries' exports, limits and argument validation, and the train.py flags."""
import ctypes
import os

import numpy as np
import pytest

import dynamic_mix as dm


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ reverb_host
@pytest.mark.parametrize("T,L", [(7, 1), (7, 5000), (300, 2), (2049, 257), (2049, 5000)])
def test_reverb_host_against_numpy_convolve(T, L):
    """Per sample (min(n + 1, L) + 3) 2^-24 sum |h x|: the sequential fp32 sum of min(n + 1, L)
    terms, the product rounding and the roundings of the two fp32 operands (§20's count)."""
    rng = np.random.default_rng(T * 7 + L)
    x = rng.uniform(-1, 1, T).astype(np.float32)
    h = (rng.standard_normal(L) * np.exp(-np.arange(L) / 700.0)).astype(np.float32)
    y = dm.reverb_host(x, h)
    assert y.dtype == np.float32 and y.shape == (T,)
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    ref = np.convolve(x64, h64)[:T]
    mag = np.convolve(np.abs(x64), np.abs(h64))[:T]
    bound = (np.minimum(np.arange(T) + 1, L) + 3) * 2.0 ** -24 * mag
    assert (bound > 0).all()
    print(f"T={T} L={L}: worst error {np.max(np.abs(y - ref) / bound):.3f} of the bound")
    assert (np.abs(y - ref) <= bound).all()


def test_reverb_host_unit_tap_returns_the_segment():
    x = np.random.default_rng(0).uniform(-1, 1, 300).astype(np.float32)
    x[5] = -0.0
    y = dm.reverb_host(x, [1.0])
    assert np.array_equal(_bits(y)[np.arange(300) != 5], _bits(x)[np.arange(300) != 5]) and y[5] == 0.0


# ------------------------------------------------------------------ plan_aug_host
LENS = [4200, 1000, 5000, 1, 3000, 1000, 2500, 4099, 999, 1200, 1700, 4100]
SPK = [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 0]
NLENS = [7, 1000, 6000, 2049, 4099]
SPEEDS = (95, 100, 105)
HALF_SEED = 11                                           # at rir_prob 0.5: dry and wet slots, also within a row


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def _plan(M, first=0, seed=HALF_SEED, speeds=None, rir_prob=0.5, T=1000, n_rirs=7, noise=True):
    off, noff = _off(LENS), _off(NLENS)
    need = T if speeds is None else max(dm.segment_span(T, *dm.speed_ratio(p)) for p in speeds)
    kw = dict(noise_off=noff, noise_elig=dm.eligible(noff, T), snr_db=(-5.0, 5.0)) if noise else {}
    return dm.plan_aug_host(off, np.asarray(SPK, np.int32), dm.eligible(off, need), M, 2, T, seed=seed,
                            first_sample=first, speeds=speeds, n_rirs=n_rirs, rir_prob=rir_prob, **kw)


@pytest.mark.parametrize("speeds", [None, SPEEDS])
def test_plan_aug_keeps_the_source_plan(speeds):
    off = _off(LENS)
    need = 1000 if speeds is None else max(dm.segment_span(1000, *dm.speed_ratio(p)) for p in speeds)
    first = (1 << 40) + 5
    a = _plan(40, first=first, speeds=speeds)
    src = dm.plan_host(off, np.asarray(SPK, np.int32), dm.eligible(off, need), 40, 2, 1000, seed=HALF_SEED,
                       first_sample=first, speeds=speeds)
    plan, idx = (src, np.zeros((40, 2), np.int32)) if speeds is None else src
    assert a["plan"].tobytes() == plan.tobytes() and np.array_equal(a["speed_idx"], idx)
    assert a["rir"].dtype == np.int32 and a["rir"].shape == (40, 2) and a["nplan"].shape == (40,)


def test_plan_aug_rir_probability_and_noise_ranges():
    assert (_plan(64, rir_prob=0.0)["rir"] == -1).all()
    always = _plan(64, rir_prob=1.0)["rir"]
    assert (always >= 0).all() and (always < 7).all() and len(set(always.ravel().tolist())) == 7
    half = _plan(8)["rir"]
    assert (half == -1).any() and (half >= 0).any()
    assert ((half == -1).any(axis=1) & (half >= 0).any(axis=1)).any(), "no row with a dry and a wet slot"
    assert (_plan(8, n_rirs=0, rir_prob=1.0)["rir"] == -1).all()
    assert _plan(8, noise=False)["nplan"] is None
    nplan = _plan(200)["nplan"]
    assert set(nplan["utt"].tolist()) == {1, 2, 3, 4} and (nplan["tries"] == 1).all()
    assert (nplan["start"] >= 0).all() and (nplan["start"] + 1000 <= np.asarray(NLENS)[nplan["utt"]]).all()
    assert (nplan["level_db"] >= -5.0).all() and (nplan["level_db"] <= 5.0).all() and np.ptp(nplan["level_db"]) > 8
    noff = _off(NLENS)
    bad = dm.plan_aug_host(_off(LENS), np.asarray(SPK, np.int32), dm.eligible(_off(LENS), 1000), 30, 2, 1000,
                           noise_off=noff, noise_elig=np.array([0, 5, -1, 2], np.int32))["nplan"]
    assert set(bad["utt"].tolist()) == {-1, 2}           # too short, == n_utts, negative: -1


def test_plan_aug_depends_on_seed_and_global_sample_only():
    whole = _plan(8, first=40, speeds=SPEEDS)
    r0, r1 = _plan(4, first=(5 * 2 + 0) * 4, speeds=SPEEDS), _plan(4, first=(5 * 2 + 1) * 4, speeds=SPEEDS)
    for f in ("plan", "speed_idx", "rir", "nplan"):
        assert np.array_equal(np.concatenate([r0[f], r1[f]]), whole[f]), f
    other = _plan(8, first=40, speeds=SPEEDS, seed=HALF_SEED + 1)
    assert not np.array_equal(other["rir"], whole["rir"]) and not np.array_equal(other["nplan"], whole["nplan"])


# ------------------------------------------------------------------ mix_aug_host
def _pool():
    rng = np.random.default_rng(0)
    pool = rng.integers(-32768, 32767, 3000).astype(np.int16)
    plan = np.array([[(0, 3, 1.5, 1), (1, 1001, -2.0, 1)], [(0, 0, 0.0, 1), (0, 902, 0.0, 1)]], dtype=dm.PLAN_DTYPE)
    return pool, np.array([0, 1000, 3000], np.int64), plan


@pytest.mark.parametrize("level_mode", [0, 1])
def test_mix_aug_host_all_off_equals_mix_host(level_mode):
    pool, off, plan = _pool()
    plain = dm.mix_host(pool, off, plan, 99, level_mode=level_mode)
    aug = dm.mix_aug_host(pool, off, plan, 99, level_mode=level_mode)
    dry = dm.mix_aug_host(pool, off, plan, 99, level_mode=level_mode, rirs=[np.ones(3, np.float32)],
                          rir=np.full((2, 2), -1, np.int32))
    assert plain["status"].tolist() == aug["status"].tolist() == dry["status"].tolist() == [0, 1]
    for f in ("gains", "p", "sources", "mixture"):
        assert plain[f].tobytes() == aug[f].tobytes() == dry[f].tobytes(), f
    assert not aug["noise"].any() and not aug["ngain"].any()
    sp = dm.mix_host(pool, off, plan, 99, level_mode=level_mode, speeds=SPEEDS, speed_idx=np.array([[0, 2], [1, 1]]))
    asp = dm.mix_aug_host(pool, off, plan, 99, level_mode=level_mode, speeds=SPEEDS, speed_idx=np.array([[0, 2], [1, 1]]))
    for f in ("gains", "p", "sources", "mixture", "status"):
        assert sp[f].tobytes() == asp[f].tobytes(), f
    for k in (-2, 1):                                    # a RIR index outside [-1, n_rirs)
        bad = dm.mix_aug_host(pool, off, plan[:1], 99, rirs=[np.ones(3, np.float32)], rir=np.array([[0, k]], np.int32))
        assert bad["status"].tolist() == [1] and not bad["sources"].any()
    with pytest.raises(ValueError, match="rir"):
        dm.mix_aug_host(pool, off, plan, 99, rirs=[np.ones(3, np.float32)])
    with pytest.raises(ValueError, match="nplan"):
        dm.mix_aug_host(pool, off, plan, 99, noise_pool=pool, noise_off=off)


@pytest.mark.parametrize("level_mode", [0, 1])
def test_mix_aug_host_achieved_snr(level_mode):
    """Before the guard (peak 0) the sources' fp32 sum is s[n] itself, so P_s is the number the
    gain was computed from; the noise power differs from g_z^2 P_z by the rounding of g_z to fp32
    and the one rounding of every fl32(g_z z[n]): each at most 2^-24 relative in amplitude, so at
    most 2 (2^-24 + 2^-24) = 2^-22 relative in power, i.e. (10 / ln 10) 2^-22 = 1.04e-6 dB; the
    fp64 sums add less than 1e-9 dB."""
    rng = np.random.default_rng(2)
    pool, off, plan = _pool()
    plan = plan[:1]
    T = 997
    zpool = (rng.uniform(-1, 1, 5000) * 0.3).astype(np.float32)
    noff = np.array([0, 2000, 5000], np.int64)
    tol = 10.0 / np.log(10.0) * 2.0 ** -22 + 1e-9
    worst = 0.0
    for snr, e in ((-5.0, (0, 1000, 0.0, 1)), (0.0, (1, 7, 0.0, 1)), (3.25, (1, 2001, 0.0, 1)), (17.5, (0, 0, 0.0, 1))):
        nplan = np.array([e], dtype=dm.PLAN_DTYPE)
        nplan["level_db"] = snr
        out = dm.mix_aug_host(pool, off, plan, T, level_mode=level_mode, peak=0.0, rirs=[np.array([1, 0.5, -0.25])],
                              rir=np.array([[0, -1]], np.int32), noise_pool=zpool, noise_off=noff, nplan=nplan)
        assert out["status"].tolist() == [0]
        s = out["sources"][0, 0] + out["sources"][0, 1]
        got = 10 * np.log10(np.mean(s.astype(np.float64) ** 2) / np.mean(out["noise"][0].astype(np.float64) ** 2))
        worst = max(worst, abs(got - snr))
        assert np.array_equal(_bits(out["mixture"][0]), _bits(s + out["noise"][0]))
    print(f"level_mode {level_mode}: achieved SNR within {worst:.2e} dB of the drawn one (tolerance {tol:.2e})")
    assert worst <= tol


def test_mix_aug_host_pool_joints_do_not_leak():
    """Loud samples before and after a RIR and a noise utterance change no bit."""
    rng = np.random.default_rng(3)
    pool, off, plan = _pool()
    T = 500
    plan = np.array([[(0, 0, 0.0, 1), (1, 1500, 1.0, 1)], [(1, 0, -1.0, 1), (0, 500, 0.5, 1)]], dtype=dm.PLAN_DTYPE)
    h = (rng.standard_normal(600) * 0.1).astype(np.float32)
    h[[0, -1]] = 1.0
    mid = rng.integers(-20000, 20000, T + 100).astype(np.int16)
    loud = lambda n: rng.choice(np.array([-32768, 32767], np.int16), n)     # noqa: E731
    noff = np.array([0, 300, 300 + len(mid), 600 + len(mid)], np.int64)
    nplan = np.array([(1, 0, 0.0, 1), (1, 100, 2.0, 1)], dtype=dm.PLAN_DTYPE)
    rir = np.array([[1, -1], [1, 1]], np.int32)
    outs = []
    for edge_h, edge_z in ((np.full(50, 9.0, np.float32), loud(300)), (np.zeros(50, np.float32), np.zeros(300, np.int16))):
        rirs = [edge_h, h, edge_h]
        zpool = np.concatenate([edge_z, mid, edge_z])
        outs.append(dm.mix_aug_host(pool, off, plan, T, level_mode=1, rirs=rirs, rir=rir, noise_pool=zpool,
                                    noise_off=noff, nplan=nplan))
    a, b = outs
    assert not a["status"].any() and a["noise"].any(axis=1).all()
    for f in ("gains", "ngain", "sources", "mixture", "noise"):
        assert a[f].tobytes() == b[f].tobytes(), f
    over = nplan.copy()
    over[1]["start"] += 1                                # start + T = len + 1
    zpool = np.concatenate([loud(300), mid, loud(300)])
    bad = dm.mix_aug_host(pool, off, plan, T, rirs=[h], rir=np.zeros((2, 2), np.int32), noise_pool=zpool,
                          noise_off=noff, nplan=over)
    assert bad["status"].tolist() == [0, 1] and not bad["mixture"][1].any() and not bad["noise"][1].any()


def test_rir_bank_and_synthetic_rir():
    import synthetic
    h = synthetic.synthetic_rir(4000, 0.3, 8000, 1)
    assert h.dtype == np.float32 and h.shape == (4000,) and h[0] == 1.0
    assert np.array_equal(h, synthetic.synthetic_rir(4000, 0.3, 8000, 1))
    assert not np.array_equal(h, synthetic.synthetic_rir(4000, 0.3, 8000, 2))
    assert np.abs(h[3000:]).max() < 0.05 * np.abs(h[1:400]).max()
    for bad in ([], [np.zeros(0)], [np.zeros(16385)]):
        with pytest.raises(ValueError):
            dm.RirBank(bad, "cpu")
    bank = dm.RirBank([np.ones(16385), np.ones(3)], "cpu", max_taps=16384)
    assert len(bank) == 2 and bank.max_len == 16384 and bank.roff_host.tolist() == [0, 16384, 16387]


def test_rir_bank_and_noise_corpus_from_wav_directories(tmp_path):
    import audio_io
    rng = np.random.default_rng(4)
    for name, n in (("b.wav", 300), ("a.wav", 50), ("notes.txt", 0)):
        if n:
            audio_io.write_wav(str(tmp_path / name), rng.uniform(-0.5, 0.5, n), 8000)
        else:
            (tmp_path / name).write_text("not a wav")
    bank = dm.RirBank.from_dir(str(tmp_path), 8000, max_taps=100, device="cpu")
    assert bank.roff_host.tolist() == [0, 50, 150] and bank.truncated == 1 and bank.max_len == 100
    a = audio_io.read_wav(str(tmp_path / "a.wav"))[0]
    assert np.array_equal(bank.rirs_host[0], a) and np.array_equal(bank.pool.numpy()[:50], a)
    noise = dm.DeviceCorpus.from_wav_dir(str(tmp_path), 8000, device="cpu")
    assert noise.n_utts == 2 and noise.off_host.tolist() == [0, 50, 350] and noise.pool_dtype == 1
    (tmp_path / "empty").mkdir()
    for load in (dm.RirBank.from_dir, dm.DeviceCorpus.from_wav_dir):
        with pytest.raises(ValueError, match="no wav"):
            load(str(tmp_path / "empty"), 8000, device="cpu")


# ------------------------------------------------------------------ C entries
def _desc(**kw):
    import ctn_lib as L
    d = dict(M=4, C=2, T=1000, n_utts=12, n_elig=9, pool_dtype=0, level_mode=0, max_tries=16, level_lo_db=-2.5,
             level_hi_db=2.5, peak=0.9, seed=1)
    d.update(kw)
    return L.DmixDesc(**d)


def _aug(**kw):
    import ctn_lib as L
    d = dict(n_rirs=7, rir_max_taps=16384, rir_prob=0.5, n_noise_utts=5, n_noise_elig=4, noise_dtype=0, snr_lo_db=-5.0,
             snr_hi_db=5.0)
    d.update(kw)
    return L.DmixAug(**d)


def _speeds(*ratios):
    import ctn_lib as L
    s = L.DmixSpeeds(n=len(ratios))
    for k, (up, down) in enumerate(ratios):
        s.r[k].up, s.r[k].down = up, down
    return s


def test_symbols_and_struct_layout(lib):
    import ctn_lib as L
    for name in ("ctn_dmix_aug_workspace_bytes", "ctn_dmix_draw_aug", "ctn_dmix_mix_aug"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(L.DmixAug) == 32 and L.DmixAug.snr_hi_db.offset == 28
    assert lib.ctn_abi_version() == 13                   # added without a version bump


def _draw(lib, d, s, g, p, **kw):
    a = dict(off=p, spk=p, elig=p, noff=p, nelig=p, plan=p, speed=p, rir=p, nplan=p)
    a.update(kw)
    return lib.ctn_dmix_draw_aug(d, s, g, a["off"], a["spk"], a["elig"], a["noff"], a["nelig"], 0, None, 0, a["plan"],
                                 a["speed"], a["rir"], a["nplan"], None)


MIX_ARGS = ("filt", "pool", "off", "plan", "speed", "rir_pool", "roff", "rir", "noise_pool", "noff", "nplan", "gains",
            "ngain", "sources", "mixture", "noise_out", "status")


def _mix(lib, d, s, g, p, ws=None, ws_bytes=1 << 40, **kw):
    a = {n: p for n in MIX_ARGS}
    a.update(kw)
    return lib.ctn_dmix_mix_aug(d, s, g, *[a[n] for n in MIX_ARGS], p if ws is None else ws, ws_bytes, None)


def test_workspace_and_error_codes_at_and_beyond_each_limit(lib):
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    sp = ctypes.byref(_speeds((20, 19), (1, 1), (20, 21)))

    def ws(d=None, s=None, **kw):
        return lib.ctn_dmix_aug_workspace_bytes(ctypes.byref(d or _desc()), s, ctypes.byref(_aug(**kw)))

    def rc(d=None, s=None, **kw):
        d, g = ctypes.byref(d or _desc()), ctypes.byref(_aug(**kw))
        a, b = _draw(lib, d, s, g, p), _mix(lib, d, s, g, p)
        assert a == b and lib.ctn_last_error().decode()
        return a

    plain = lib.ctn_dmix_workspace_bytes(ctypes.byref(_desc()))
    assert ws(n_rirs=0, n_noise_utts=0, n_noise_elig=0) == plain
    assert ws(s=sp, n_rirs=0, n_noise_utts=0, n_noise_elig=0) == lib.ctn_dmix_sp_workspace_bytes(ctypes.byref(_desc()), sp)
    assert ws() >= plain + 4 * 2 * 1000 * 4 + 8 * 16 + 9 * 8 + 4 * 1 * 16 + 4 * 4      # xv, its tables, powers, g_z
    assert ws(s=sp) >= ws() + 4 * 2 * 1000 * 4
    assert ws(rir_max_taps=16384) > 0 and ws(rir_max_taps=1) > 0
    assert ws(d=_desc(C=15)) > 0 and ws(d=_desc(C=16), n_noise_utts=0, n_noise_elig=0) > 0
    assert ws(rir_prob=0.0) > 0 and ws(rir_prob=1.0) > 0
    for kw, code, word in ((dict(rir_max_taps=16385), 2, "limits"), (dict(rir_max_taps=0), 1, "rir_max_taps"),
                           (dict(rir_prob=-0.01), 1, "rir_prob"), (dict(rir_prob=1.01), 1, "rir_prob"),
                           (dict(rir_prob=float("nan")), 1, "rir_prob"), (dict(snr_lo_db=float("inf")), 1, "finite"),
                           (dict(snr_hi_db=float("nan")), 1, "finite"), (dict(noise_dtype=2), 1, "noise_dtype"),
                           (dict(n_rirs=-1), 1, "n_rirs"), (dict(n_noise_elig=0), 1, "n_noise_elig"),
                           (dict(n_noise_utts=0), 1, "n_noise_elig")):
        assert ws(**kw) == 0, kw
        assert rc(**kw) == code, kw
        assert word in lib.ctn_last_error().decode(), (kw, lib.ctn_last_error().decode())
    assert ws(d=_desc(C=16)) == 0 and rc(d=_desc(C=16)) == 2 and "limits" in lib.ctn_last_error().decode()
    assert ws(d=_desc(C=17), n_noise_utts=0, n_noise_elig=0) == 0
    assert ws(s=ctypes.byref(_speeds((3, 1)))) == 0 and rc(s=ctypes.byref(_speeds((3, 1)))) == 2
    assert lib.ctn_dmix_aug_workspace_bytes(None, None, ctypes.byref(_aug())) == 0
    assert lib.ctn_dmix_aug_workspace_bytes(ctypes.byref(_desc()), None, None) == 0


def test_entries_validate_before_the_device(lib):
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    d, s, g = ctypes.byref(_desc()), ctypes.byref(_speeds((20, 19), (1, 1))), ctypes.byref(_aug())
    assert _draw(lib, None, s, g, p) == 1 and _draw(lib, d, s, None, p) == 1
    assert _mix(lib, None, s, g, p) == 1 and _mix(lib, d, s, None, p) == 1
    for name in ("off", "spk", "elig", "noff", "nelig", "plan", "speed", "rir", "nplan"):
        assert _draw(lib, d, s, g, p, **{name: None}) == 1, name
        assert "null pointer" in lib.ctn_last_error().decode()
    for name in MIX_ARGS:
        if name == "noise_out":
            continue                                     # optional
        assert _mix(lib, d, s, g, p, **{name: None}) == 1, name
        assert "null pointer" in lib.ctn_last_error().decode()
    assert _mix(lib, d, s, g, p, ws=0, ws_bytes=0) == 3                                  # no workspace
    need = lib.ctn_dmix_aug_workspace_bytes(d, s, g)
    assert _mix(lib, d, s, g, p, ws_bytes=need - 1) == 3 and "workspace" in lib.ctn_last_error().decode()
    assert _mix(lib, d, s, g, p, ws_bytes=lib.ctn_dmix_sp_workspace_bytes(d, s)) == 3    # what _sp needs is not enough
    assert _mix(lib, d, s, g, p, ws=p + 8) == 1 and "aligned" in lib.ctn_last_error().decode()
    for name, by in (("pool", 1), ("rir_pool", 2), ("noise_pool", 1), ("roff", 4), ("noff", 4), ("noise_out", 2),
                     ("sources", 2), ("mixture", 2), ("filt", 2)):
        assert _mix(lib, d, s, g, p, **{name: p + by}) == 1, name
        assert "aligned" in lib.ctn_last_error().decode()
    for bad, code in ((dict(C=0), 1), (dict(T=0), 1), (dict(C=17), 2), (dict(max_tries=65), 2)):
        b = ctypes.byref(_desc(**bad))
        assert _draw(lib, b, s, g, p) == code and _mix(lib, b, s, g, p) == code, bad


# ------------------------------------------------------------------ Python surface
def test_train_parser_dm_aug_flags(tmp_path):
    import train
    a = train.parser.parse_args([])
    assert a.dm_rir_dir == "" and a.dm_noise_dir == "" and a.dm_rir_prob == 1.0 and a.dm_rir_max_taps == 16384
    assert a.dm_snr_db == [-5.0, 5.0]
    train.check_dm_aug(a)
    a = train.parser.parse_args(["--dynamic_mix", "1", "--dm_rir_dir", str(tmp_path), "--dm_rir_prob", "0.5",
                                 "--dm_rir_max_taps", "4000", "--dm_noise_dir", str(tmp_path), "--dm_snr_db", "-3", "6",
                                 "--use_cuda", "0"])
    assert (a.dm_rir_prob, a.dm_rir_max_taps, a.dm_snr_db) == (0.5, 4000, [-3.0, 6.0])
    train.check_dm_aug(a)
    with pytest.raises(ValueError, match="use_cuda"):    # accepted; dynamic mixing itself needs the GPU
        train.main(a)
    for flag in ("--dm_rir_dir", "--dm_noise_dir"):
        with pytest.raises(ValueError, match="dynamic_mix 1"):
            train.main(train.parser.parse_args([flag, str(tmp_path)]))
    for bad in (["--dm_rir_prob", "1.5"], ["--dm_rir_max_taps", "16385"], ["--dm_rir_max_taps", "0"],
                ["--dm_snr_db", "0", "inf"]):
        with pytest.raises(ValueError, match=bad[0][2:]):
            train.main(train.parser.parse_args(["--dynamic_mix", "1"] + bad))
