"""Speed perturbation of dynamic mixing (dynamic_mix.py; ctn_dmix_draw_sp / ctn_dmix_mix_sp)
checks that need no GPU: the filter design and the host resampler against scipy, the rule
at utterance ends, the properties of the host plan with speeds, the C entries' exports,
limits and argument validation, and the train.py flag."""
import ctypes
import os

import numpy as np
import pytest

import dynamic_mix as dm

RATIOS = [(20, 19), (20, 21), (10, 9), (10, 11), (2, 1), (1, 2)]
N = 6000


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


@pytest.fixture(scope="module")
def utterance():
    """A whole PCM16 utterance of N samples as exact fp32 values."""
    s = np.random.default_rng(1).integers(-32768, 32768, N).astype(np.int16)
    return s.astype(np.float32) * np.float32(2.0 ** -15)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------ ratios and filter
def test_speed_ratio_and_span():
    assert dm.speed_ratio(95) == (20, 19) and dm.speed_ratio(105) == (20, 21) and dm.speed_ratio(100) == (1, 1)
    assert dm.speed_ratio(50) == (2, 1) and dm.speed_ratio(200) == (1, 2) and dm.speed_ratio(110) == (10, 11)
    for bad in (49, 201, 97, 0, -5, 99.5):               # beyond 1/2..2, up = 100 > 64, not a positive integer
        with pytest.raises(ValueError):
            dm.speed_ratio(bad)
    assert dm.segment_span(1, 20, 19) == 1 and dm.segment_span(1000, 1, 1) == 1000
    assert dm.segment_span(1000, 20, 19) == 999 * 19 // 20 + 1 == 950
    assert dm.segment_span(1000, 20, 21) == 1049 and dm.segment_span(7, 1, 2) == 13


@pytest.mark.parametrize("up,down", RATIOS)
def test_filter_is_the_resample_poly_design(up, down):
    """fp64 rounding only between the numpy design and scipy's firwin: 1e-12 of the largest tap."""
    signal = pytest.importorskip("scipy.signal")
    h64, hl = dm._speed_filter64(up, down)
    assert hl == 10 * max(up, down) and len(h64) == 2 * hl + 1
    ref = signal.firwin(2 * hl + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    err = np.abs(h64 - ref).max() / np.abs(ref).max()
    print(f"{up}/{down}: filter differs from firwin by {err:.2e} of the largest tap")
    assert err <= 1e-12
    h32, hl32 = dm.speed_filter(up, down)
    assert hl32 == hl and h32.dtype == np.float32 and np.array_equal(h32, h64.astype(np.float32))


def _bound(x, start, T, up, down):
    """(ntap + 3) 2^-24 sum_i |h x| per output: the sequential fp32 sum of ntap terms, the
    product rounding and the coefficient rounding, against exact arithmetic."""
    h, hl = dm._speed_filter64(up, down)
    t = np.arange(T, dtype=np.int64) * down + hl
    mag = np.zeros(T)
    ntap = 2 * hl // up + 1
    for j in range(ntap):
        hi, a = t % up + j * up, start + t // up - j
        ok = (hi <= 2 * hl) & (a >= 0) & (a < len(x))
        mag += np.where(ok, np.abs(h[np.where(ok, hi, 0)] * x[np.where(ok, a, 0)].astype(np.float64)), 0.0)
    return (ntap + 3) * 2.0 ** -24 * mag


@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_host_whole_utterance_against_scipy(utterance, up, down):
    signal = pytest.importorskip("scipy.signal")
    y64 = signal.resample_poly(utterance.astype(np.float64), up, down)
    T = -(-N * up // down)
    assert len(y64) == T
    y = dm.resample_host(utterance, 0, T, up, down)
    assert y.dtype == np.float32 and y.shape == (T,)
    bound = _bound(utterance, 0, T, up, down)
    assert (bound > 0).all()
    print(f"{up}/{down}: worst error {np.max(np.abs(y - y64) / bound):.3f} of the bound")
    assert (np.abs(y - y64) <= bound).all()


@pytest.mark.parametrize("up,down", RATIOS)
def test_resample_host_interior_segment_uses_real_neighbours(utterance, up, down):
    """A segment whose start is a multiple of `down` is a slice of the whole utterance's
    resampling: the samples before and after it feed the filter's tails."""
    signal = pytest.importorskip("scipy.signal")
    y64 = signal.resample_poly(utterance.astype(np.float64), up, down)
    start = 100 * down
    T = 1000
    assert start + dm.segment_span(T, up, down) <= N
    y = dm.resample_host(utterance, start, T, up, down)
    first = start * up // down
    assert (np.abs(y - y64[first:first + T]) <= _bound(utterance, start, T, up, down)).all()


def test_resample_host_unit_ratio_is_the_segment(utterance):
    assert np.array_equal(_bits(dm.resample_host(utterance, 17, 500, 1, 1)), _bits(utterance[17:517]))
    assert np.array_equal(dm.resample_host(utterance, N - 2, 4, 1, 1), [utterance[-2], utterance[-1], 0, 0])


# ------------------------------------------------------------------ utterance ends
@pytest.mark.parametrize("speeds", [(95, 105), (50, 200)])
def test_neighbouring_utterances_do_not_leak(speeds):
    """Full-scale noise before and after an utterance changes no bit of a segment at its
    first sample or at len - span."""
    rng = np.random.default_rng(3)
    T, n1 = 300, 700
    noise = lambda n: rng.choice(np.array([-32768, 32767], np.int16), n)     # noqa: E731
    mid = rng.integers(-20000, 20000, n1).astype(np.int16)
    off = np.array([0, 500, 500 + n1, 1000 + n1], np.int64)
    loud = np.concatenate([noise(500), mid, noise(500)])
    quiet = np.concatenate([np.zeros(500, np.int16), mid, np.zeros(500, np.int16)])
    spans = [dm.segment_span(T, *dm.speed_ratio(p)) for p in speeds]
    plan = np.array([[(1, 0, 0.0, 1), (1, n1 - spans[0], 1.0, 1)],
                     [(1, 0, -1.0, 1), (1, n1 - spans[1], 0.5, 1)]], dtype=dm.PLAN_DTYPE)
    idx = np.array([[0, 0], [1, 1]], np.int32)
    a = dm.mix_host(loud, off, plan, T, speeds=speeds, speed_idx=idx)
    b = dm.mix_host(quiet, off, plan, T, speeds=speeds, speed_idx=idx)
    assert not a["status"].any() and a["sources"].any(axis=2).all()
    assert np.array_equal(_bits(a["sources"]), _bits(b["sources"]))
    assert np.array_equal(_bits(a["mixture"]), _bits(b["mixture"]))
    over = plan.copy()
    over[1, 1]["start"] += 1                             # start + span = len + 1
    assert dm.mix_host(loud, off, over, T, speeds=speeds, speed_idx=idx)["status"].tolist() == [0, 1]


# ------------------------------------------------------------------ plan and mix
def _corpus(lens, spk):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(spk, np.int32)


LENS = [4200, 1000, 5000, 1, 3000, 1000, 2500, 4099, 999, 1200, 1700, 4100]
SPK = [0, 0, 1, 0, 0, 2, 0, 0, 1, 0, 0, 0]
SPEEDS = (95, 100, 105)


def _elig(off, T, speeds):
    return dm.eligible(off, max(dm.segment_span(T, *dm.speed_ratio(p)) for p in speeds))


def test_plan_with_unit_speed_is_the_plain_plan():
    off, spk = _corpus(LENS, SPK)
    elig = dm.eligible(off, 1000)
    plain = dm.plan_host(off, spk, elig, 40, 2, 1000, seed=3, first_sample=(1 << 40) + 5)
    plan, idx = dm.plan_host(off, spk, elig, 40, 2, 1000, seed=3, first_sample=(1 << 40) + 5, speeds=[100])
    assert plan.tobytes() == plain.tobytes() and idx.dtype == np.int32 and not idx.any()


def test_plan_with_speeds_indices_and_ranges():
    off, spk = _corpus(LENS, SPK)
    T = 1000
    elig = _elig(off, T, SPEEDS)
    assert elig.tolist() == [i for i, n in enumerate(LENS) if n >= 1049]
    plan, idx = dm.plan_host(off, spk, elig, 300, 2, T, seed=3, speeds=SPEEDS)
    assert plan.shape == idx.shape == (300, 2)
    assert sorted(set(idx.ravel().tolist())) == [0, 1, 2]
    spans = np.array([dm.segment_span(T, *dm.speed_ratio(p)) for p in SPEEDS])
    assert spans.tolist() == [950, 1000, 1049]
    n = np.diff(off)[plan["utt"]]
    assert (plan["start"] >= 0).all() and (plan["start"] + spans[idx] <= n).all()
    assert (plan["tries"] > 1).any()


def test_plan_with_speeds_depends_on_seed_and_global_sample_only():
    off, spk = _corpus(LENS, SPK)
    elig = _elig(off, 1000, SPEEDS)
    kw = dict(C=2, T=1000, seed=11, speeds=SPEEDS)
    whole = dm.plan_host(off, spk, elig, M=8, first_sample=40, **kw)
    r0 = dm.plan_host(off, spk, elig, M=4, first_sample=(5 * 2 + 0) * 4, **kw)
    r1 = dm.plan_host(off, spk, elig, M=4, first_sample=(5 * 2 + 1) * 4, **kw)
    for i in (0, 1):
        assert np.array_equal(np.concatenate([r0[i], r1[i]]), whole[i])
    one = dm.plan_host(off, spk, elig, M=1, first_sample=43, **kw)
    assert np.array_equal(one[0][0], whole[0][3]) and np.array_equal(one[1][0], whole[1][3])
    other = dm.plan_host(off, spk, elig, M=8, first_sample=40, C=2, T=1000, seed=12, speeds=SPEEDS)
    assert not np.array_equal(other[0], whole[0])


@pytest.mark.parametrize("level_mode", [0, 1])
def test_mix_host_all_unit_slots_equal_the_plain_mix(level_mode):
    rng = np.random.default_rng(0)
    pool = rng.integers(-32768, 32767, 3000).astype(np.int16)
    off = np.array([0, 1000, 3000], np.int64)
    plan = np.array([[(0, 3, 1.5, 1), (1, 1001, -2.0, 1)], [(0, 0, 0.0, 1), (0, 902, 0.0, 1)]], dtype=dm.PLAN_DTYPE)
    plain = dm.mix_host(pool, off, plan, 99, level_mode=level_mode)
    sp = dm.mix_host(pool, off, plan, 99, level_mode=level_mode, speeds=SPEEDS, speed_idx=np.ones((2, 2), np.int32))
    assert plain["status"].tolist() == sp["status"].tolist() == [0, 1]
    for f in ("gains", "p", "sources", "mixture"):
        assert plain[f].tobytes() == sp[f].tobytes(), f
    bad = dm.mix_host(pool, off, plan, 99, speeds=SPEEDS, speed_idx=np.array([[1, 3], [1, 1]], np.int32))
    assert bad["status"].tolist() == [1, 1]              # speed index == S
    with pytest.raises(ValueError, match="speed_idx"):
        dm.mix_host(pool, off, plan, 99, speeds=SPEEDS)


# ------------------------------------------------------------------ C entries
def _desc(**kw):
    import ctn_lib as L
    d = dict(M=4, C=2, T=1000, n_utts=12, n_elig=9, pool_dtype=0, level_mode=0, max_tries=16, level_lo_db=-2.5,
             level_hi_db=2.5, peak=0.9, seed=1)
    d.update(kw)
    return L.DmixDesc(**d)


def _speeds(*ratios, n=None):
    import ctn_lib as L
    s = L.DmixSpeeds(n=len(ratios) if n is None else n)
    for k, (up, down) in enumerate(ratios):
        s.r[k].up, s.r[k].down = up, down
    return s


def test_symbols_and_table_layout(lib):
    import ctn_lib as L
    for name in ("ctn_dmix_sp_filter_floats", "ctn_dmix_sp_workspace_bytes", "ctn_dmix_draw_sp", "ctn_dmix_mix_sp"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert ctypes.sizeof(L.DmixSpeeds) == 68 and L.DmixSpeeds.r.offset == 4
    assert lib.ctn_abi_version() == 13                   # added without a version bump


def test_filter_floats(lib):
    ff = lambda *r, **kw: lib.ctn_dmix_sp_filter_floats(ctypes.byref(_speeds(*r, **kw)))   # noqa: E731
    assert ff((20, 19)) == 401 and ff((20, 21)) == 421 and ff((1, 1)) == 0
    assert ff((20, 19), (1, 1), (20, 21)) == 822
    assert ff(*[(64, 63)] * 8) == 8 * 1281
    assert ff(n=0) == 0 and ff(*[(1, 1)] * 8, n=9) == 0 and lib.ctn_dmix_sp_filter_floats(None) == 0
    for up, down in RATIOS:
        assert ff((up, down)) == len(dm.speed_filter(up, down)[0])


def test_workspace_and_error_codes_at_and_beyond_each_limit(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    d = _desc()
    plain = lib.ctn_dmix_workspace_bytes(ctypes.byref(d))

    def ws(*r, **kw):
        return lib.ctn_dmix_sp_workspace_bytes(ctypes.byref(d), ctypes.byref(_speeds(*r, **kw)))

    def rc(*r, **kw):
        s = _speeds(*r, **kw)
        a = lib.ctn_dmix_draw_sp(ctypes.byref(d), ctypes.byref(s), p, p, p, 0, None, 0, p, p, None)
        b = lib.ctn_dmix_mix_sp(ctypes.byref(d), ctypes.byref(s), p, p, p, p, p, p, p, p, p, p, 1 << 40, None)
        assert a == b and lib.ctn_last_error().decode()
        return a

    # xr [M][C][T] fp32 and the tables that present it to the mix kernels come on top
    assert ws((20, 19), (1, 1), (20, 21)) >= plain + 4 * 2 * 1000 * 4 + 8 * 16 + 9 * 8
    for ok in ([(1, 1)], [(1, 1)] * 8, [(64, 63)], [(63, 64)], [(2, 1)], [(1, 2)], [(33, 64)], [(64, 33)]):
        assert ws(*ok) > 0, ok
    for r, kw, code in (((), dict(n=0), 1), ([(1, 1)] * 8, dict(n=9), 2), ([(65, 64)], {}, 2), ([(64, 65)], {}, 2),
                        ([(0, 1)], {}, 1), ([(1, 0)], {}, 1), ([(4, 2)], {}, 1), ([(20, 20)], {}, 1),
                        ([(3, 1)], {}, 2), ([(1, 3)], {}, 2), ([(63, 31)], {}, 2), ([(31, 63)], {}, 2),
                        ([(1, 1), (20, 19), (5, 2)], {}, 2)):
        assert ws(*r, **kw) == 0, (r, kw)
        assert rc(*r, **kw) == code, (r, kw)
    assert lib.ctn_dmix_sp_workspace_bytes(None, ctypes.byref(_speeds((1, 1)))) == 0
    assert lib.ctn_dmix_sp_workspace_bytes(ctypes.byref(d), None) == 0
    assert lib.ctn_dmix_sp_workspace_bytes(ctypes.byref(_desc(C=17)), ctypes.byref(_speeds((1, 1)))) == 0


def test_entries_validate_before_the_device(lib):
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    d, s = ctypes.byref(_desc()), ctypes.byref(_speeds((20, 19), (1, 1)))
    assert lib.ctn_dmix_draw_sp(None, s, p, p, p, 0, None, 0, p, p, None) == 1
    assert lib.ctn_dmix_draw_sp(d, None, p, p, p, 0, None, 0, p, p, None) == 1
    assert lib.ctn_dmix_mix_sp(None, s, *[p] * 9, p, 1 << 40, None) == 1
    assert lib.ctn_dmix_mix_sp(d, None, *[p] * 9, p, 1 << 40, None) == 1
    for i in range(5):                                   # off, spk, elig, plan, speed
        a = [p, p, p, 0, None, 0, p, p]
        a[i if i < 3 else i + 3] = None
        assert lib.ctn_dmix_draw_sp(d, s, *a, None) == 1
        assert "null pointer" in lib.ctn_last_error().decode()
    for i in range(9):                                   # filt, pool, off, plan, speed, gains, sources, mixture, status
        a = [p] * 9
        a[i] = None
        assert lib.ctn_dmix_mix_sp(d, s, *a, p, 1 << 40, None) == 1, i
        assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_dmix_mix_sp(d, s, *[p] * 9, None, 0, None) == 3                      # no workspace
    need = lib.ctn_dmix_sp_workspace_bytes(d, s)
    assert lib.ctn_dmix_mix_sp(d, s, *[p] * 9, p, need - 1, None) == 3                  # short workspace
    assert "workspace" in lib.ctn_last_error().decode()
    # what the plain mix needs is not enough
    assert lib.ctn_dmix_mix_sp(d, s, *[p] * 9, p, lib.ctn_dmix_workspace_bytes(d), None) == 3
    a = [p] * 9
    a[1] = p + 1                                         # pool
    assert lib.ctn_dmix_mix_sp(d, s, *a, p, 1 << 40, None) == 1
    assert "aligned" in lib.ctn_last_error().decode()
    for bad, code in ((dict(C=0), 1), (dict(T=0), 1), (dict(C=17), 2), (dict(max_tries=65), 2)):
        b = ctypes.byref(_desc(**bad))
        assert lib.ctn_dmix_draw_sp(b, s, p, p, p, 0, None, 0, p, p, None) == code, bad
        assert lib.ctn_dmix_mix_sp(b, s, *[p] * 9, p, 1 << 40, None) == code, bad


# ------------------------------------------------------------------ Python surface
def test_train_parser_dm_speeds():
    import train
    assert train.parser.parse_args([]).dm_speeds == [100]
    train.check_dm_speeds(train.parser.parse_args([]))
    a = train.parser.parse_args(["--dynamic_mix", "1", "--dm_speeds", "95", "100", "105", "--use_cuda", "0"])
    assert a.dm_speeds == [95, 100, 105]
    train.check_dm_speeds(a)
    with pytest.raises(ValueError, match="use_cuda"):    # accepted; dynamic mixing itself needs the GPU
        train.main(a)
    with pytest.raises(ValueError, match="dynamic_mix 1"):
        train.main(train.parser.parse_args(["--dm_speeds", "95", "105"]))
    with pytest.raises(ValueError, match="dm_speeds.*49"):
        train.main(train.parser.parse_args(["--dynamic_mix", "1", "--dm_speeds", "49", "100"]))
    with pytest.raises(ValueError, match="dm_speeds"):
        train.main(train.parser.parse_args(["--dynamic_mix", "1", "--dm_speeds"] + ["100"] * 9))
