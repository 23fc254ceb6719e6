"""PIT with silent sources without a GPU: the fp64 host restatement
(pit_var_criterion.pit_var_host) against the autograd twin and the PIT oracle, the margins and
tie rule that make the GPU tests' exact permutation comparison legitimate, wrong variants of
the definition, the mixer's speaker-count draw (dynamic_mix.thin_host), the C-ABI's argument
validation and the train.py / evaluate.py flags."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import pitvar_cases as K

FWD_BOUND = lambda ref: 2.0 ** -23 * abs(ref) + 1e-7      # the GPU tests' forward bound


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


def _host(case, s, e, x, lens, **kw):
    import pit_var_criterion as pv
    return pv.pit_var_host(s, e, lens, x, case["mode"], case["snr_max"], case["inactive_snr_max"], **kw)


PLANTED = [c for c in K.CASES if c["planted_perm"] and c["C"] <= 5]


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_host_agrees_with_twin_at_planted_permutation(case):
    """Two statements of one definition: numpy sample by sample, torch fp64 autograd.  The
    host's best permutation is the planted one (canonical over the silent references)."""
    s, e, x, lens, planted = K.build(case)
    h = _host(case, s, e, x, lens)
    assert np.array_equal(h["perm"], planted.numpy())
    assert np.array_equal(h["active"], np.array([[j not in sil for j in range(case["C"])] for sil in case["silent"]]))
    ms, loss, _, pairs = K.twin(s, e, lens, x, planted, case["mode"], case["snr_max"], case["inactive_snr_max"])
    assert np.abs(ms.numpy() - h["max_snr"]).max() < 1e-9 and abs(loss - h["loss"]) < 1e-9
    for m in range(case["M"]):
        for i in range(case["C"]):
            assert abs(float(pairs[m, i]) - h["scores"][m, i, int(planted[m, i])]) < 1e-9


@pytest.mark.parametrize("C", [2, 3, 4])
def test_all_active_si_snr_is_the_pit_oracle(C):
    """Every reference active, si_snr: max_snr and the permutation are the fp64 PIT oracle's
    (sources zero beyond the lengths, where the oracle's mean over all t is the mean over
    t < length)."""
    import pit_var_criterion as pv
    from oracle import ctn_oracle as O
    s, e, _, planted = K.planted(C, 3, 200, seed=50 + C, mixture="none")
    lens = torch.tensor([200, 151, 77])
    for m, n in enumerate(lens):
        s[m, :, n:] = 0
    h = pv.pit_var_host(s, e, lens, None, "si_snr")
    max_snr, perms, idx, _ = O.si_snr_pit(s.double(), e.double(), lens)
    assert np.array_equal(h["perm"], perms[idx].numpy()) and np.array_equal(h["perm"], planted.numpy())
    assert np.abs(h["max_snr"] - max_snr[:, 0].numpy()).max() < 1e-9
    assert h["active"].all()


def _all_cases():
    for case in K.CASES:
        yield (case,) + K.build(case)
    for kind in ("negzero", "beyond", "tiny"):
        yield K.special(kind)


def test_margins_and_first_rank_of_every_shared_case():
    """For every row of every case that test_gpu_pitvar.py compares exactly: the best
    permutation sum leads the next *distinct* sum by >= 1e-3 dB (a thousand times the forward
    bound), the permutations that share the best sum share it bit for bit (they differ only in
    which silent reference, or which -80 dB pair, an output takes), and the host returns the
    first of them in itertools order."""
    worst = math.inf
    for case, s, e, x, lens, _ in _all_cases():
        C = case["C"]
        if C > 5 and case["M"] > 1:
            continue                                 # C = 8 planted: walked once below, vectorised
        h = _host(case, s, e, x, lens)
        table = K.perm_table(C)
        for m in range(case["M"]):
            sc = h["scores"][m]
            sums = sc[np.arange(C)[None, :], table].sum(1)
            best = sums.max()
            tied = np.nonzero(sums >= best - 1e-9)[0]
            rest = np.delete(sums, tied)
            if len(rest):
                worst = min(worst, best - rest.max())
                assert best - rest.max() >= 1e-3, (case["name"], m, best - rest.max())
            seq = []
            for r in tied:                           # the search's own summation order
                v = 0.0
                for i in range(C):
                    v += sc[i, table[r, i]]
                seq.append(v)
            assert len(set(seq)) == 1, (case["name"], m, "tied sums differ in their bits")
            assert h["perm"][m].tolist() == table[tied[0]].tolist(), (case["name"], m)
            k = sum(1 for j in range(C) if not h["active"][m, j])
            if case["mode"] == "snr" and case["lengths"][m] > 1:
                assert len(tied) == math.factorial(k), (case["name"], m, len(tied), k)
    print(f"smallest margin to the next distinct permutation sum: {worst:.3g} dB")


def test_c8_planted_margins():
    """The C = 8 planted cases (40320 permutations): the same margin and first-rank checks from
    the twin's score matrix, vectorised; 7 silent references tie 5040 permutations."""
    table = K.perm_table(8)
    for case in (c for c in K.CASES if c["C"] == 8 and c["M"] > 1):
        s, e, x, lens, planted = K.build(case)
        scores = K.twin_matrix(s, e, lens, x, case["mode"], case["snr_max"], case["inactive_snr_max"])
        for m in range(case["M"]):
            sums = scores[m][np.arange(8)[None, :], table].sum(1)
            tied = np.nonzero(sums >= sums.max() - 1e-9)[0]
            assert len(tied) == math.factorial(len(case["silent"][m]))
            assert sums.max() - np.delete(sums, tied).max() >= 1e-3
            assert table[tied[0]].tolist() == planted[m].tolist()


def test_tie_cases_return_the_first_rank():
    """All references silent: every permutation ties and the identity (rank 0) is returned;
    two silent references: of the two tied permutations the lower rank."""
    for name in ("all-silent-noise-mix", "all-silent-no-mix"):
        case = next(c for c in K.CASES if c["name"] == name)
        s, e, x, lens, _ = K.build(case)
        h = _host(case, s, e, x, lens)
        assert h["perm"].tolist() == [list(range(case["C"]))] * case["M"] and not h["active"].any()
        assert np.isfinite(h["scores"]).all()
    s, e, x, planted = K.planted(3, 1, 100, seed=9, silent=[(0, 2)])
    import pit_var_criterion as pv
    h = pv.pit_var_host(s, e, torch.tensor([100]), x)
    i, k = [i for i in range(3) if planted[0, i] != 1]
    assert i < k and h["perm"][0, i] == 0 and h["perm"][0, k] == 2
    _, _, sums = K.search(h["scores"][0])
    assert np.sort(sums)[-1] == np.sort(sums)[-2]


# ---- wrong variants: each moves max_snr (or the permutation) at the case built for it ---------
def _variant(case, s, e, x, lens, variant=None, last=False):
    sc = K.twin_matrix(s, e, lens, x, case["mode"], case["snr_max"], case["inactive_snr_max"], variant=variant)
    res = [K.search(sc[m], last=last) for m in range(case["M"])]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def test_twin_search_is_the_host():
    case = next(c for c in K.CASES if c["name"] == "planted-snr-C4")
    s, e, x, lens, _ = K.build(case)
    h = _host(case, s, e, x, lens)
    perm, ms = _variant(case, s, e, x, lens)
    assert np.array_equal(perm, h["perm"]) and np.abs(ms - h["max_snr"]).max() < 1e-9


def test_wrong_silent_reference_scored_as_active():
    case = next(c for c in K.CASES if c["name"] == "planted-snr-C3")
    s, e, x, lens, _ = K.build(case)
    h = _host(case, s, e, x, lens)
    _, ms = _variant(case, s, e, x, lens, "active_formula")
    assert abs(ms[0] - h["max_snr"][0]) < 1e-9                     # all active: nothing to get wrong
    for m in (1, 2):
        assert abs(ms[m] - h["max_snr"][m]) > 1e3 * FWD_BOUND(h["max_snr"][m]), (m, ms[m], h["max_snr"][m])


def test_wrong_activity_by_threshold():
    case, s, e, x, lens, _ = K.special("tiny")
    h = _host(case, s, e, x, lens)
    assert h["active"][1, 1] and h["active"][2, 1]                  # 1e-6 N(0,1); one denormal sample
    _, ms = _variant(case, s, e, x, lens, "threshold")
    for m in (1, 2):
        assert abs(ms[m] - h["max_snr"][m]) > 1e3 * FWD_BOUND(h["max_snr"][m]), (m, ms[m], h["max_snr"][m])
    case, s, e, x, lens, _ = K.special("negzero")
    h = _host(case, s, e, x, lens)
    assert not h["active"][1, 1]
    case, s, e, x, lens, _ = K.special("beyond")
    h = _host(case, s, e, x, lens)
    assert not h["active"][1, 1] and not h["active"][2, 1]


def test_wrong_mixture_energy_from_the_sources():
    case = next(c for c in K.CASES if c["name"] == "planted-snr-C4")   # mixture = sum + 0.5 noise
    s, e, x, lens, _ = K.build(case)
    h = _host(case, s, e, x, lens)
    _, ms = _variant(case, s, e, x, lens, "x_from_sources")
    assert abs(ms[0] - h["max_snr"][0]) < 1e-9                     # no silent reference: X is not read
    for m in (1, 2):
        assert abs(ms[m] - h["max_snr"][m]) > 1e3 * FWD_BOUND(h["max_snr"][m]), (m, ms[m], h["max_snr"][m])


def test_wrong_last_maximum():
    """The tied permutations share max_snr by construction, so the last maximum shows in the
    permutation alone: it differs on every row with two or more silent references."""
    case = next(c for c in K.CASES if c["name"] == "planted-snr-C4")
    s, e, x, lens, _ = K.build(case)
    h = _host(case, s, e, x, lens)
    perm, ms = _variant(case, s, e, x, lens, last=True)
    assert np.abs(ms - h["max_snr"]).max() < 1e-9
    assert np.array_equal(perm[:2], h["perm"][:2]) and not np.array_equal(perm[2], h["perm"][2])


def test_restated_coefficient_form_against_twin():
    """The backward's coefficient form (fp32 coefficients, fp64 evaluation, one rounding)
    reproduces the fp64 autograd gradient for all three score kinds within
    test_gpu_pitvar.py's gradient bound; zero beyond each length."""
    from test_gpu_pitvar import GRAD_BOUND
    for name in ("planted-snr-C4", "planted-si_snr-C4", "threshold-regime"):
        case = next(c for c in K.CASES if c["name"] == name)
        s, e, x, lens, planted = K.build(case)
        w_loss, w_max = K.weights(case["M"])
        args = (s, e, lens, x, planted, case["mode"], case["snr_max"], case["inactive_snr_max"], w_loss, w_max)
        g = K.twin(*args)[2]
        r = K.restated_grad(*args)
        assert not r[1, :, 263:].any() and not g[2, :, 226:].any()
        assert K.row_ratio(r, g) <= GRAD_BOUND, name


# ---- the mixer's speaker count ---------------------------------------------------------------
def _corpus(n_utts=12, n_spk=6, seed=0):
    rng = np.random.default_rng(seed)
    waves = [(rng.standard_normal(int(rng.integers(3000, 5000))) * 3000).astype(np.int16) for _ in range(n_utts)]
    off = np.concatenate([[0], np.cumsum([len(w) for w in waves])]).astype(np.int64)
    spk = np.array([u % n_spk for u in range(n_utts)], np.int32)
    return np.concatenate(waves), off, spk


def test_thin_host_plan_count_and_rank_splits():
    import dynamic_mix as dm
    pool, off, spk = _corpus()
    M, C, T, seed = 256, 4, 2049, 20211
    elig = dm.eligible(off, T)
    base = dm.plan_host(off, spk, elig, M, C, T, seed=seed, first_sample=1000)
    for k in (1, 2, 3):
        plan, count = dm.thin_host(base, M, C, seed, 1000, k)
        assert count.dtype == np.int32 and sorted(set(count.tolist())) == list(range(k, C + 1)), k
        for m in range(M):
            n = int(count[m])
            assert plan[m, :n].tobytes() == base[m, :n].tobytes()
            assert np.all(np.isneginf(plan["level_db"][m, n:]))
            for f in ("utt", "start", "tries"):
                assert np.array_equal(plan[f][m, n:], base[f][m, n:])
    plan, count = dm.thin_host(base, M, C, seed, 1000, C)            # min = C: nothing is thinned
    assert plan.tobytes() == base.tobytes() and (count == C).all()
    assert np.isfinite(base["level_db"]).all()                       # the input is not written
    # the count is a function of (seed, global sample): rank splits agree with the unsplit batch
    whole = dm.thin_host(base, M, C, seed, 1000, 1)
    for world in (2, 4):
        per = M // world
        for rank in range(world):
            sl = slice(rank * per, (rank + 1) * per)
            part = dm.plan_host(off, spk, elig, per, C, T, seed=seed, first_sample=1000 + rank * per)
            p, c = dm.thin_host(part, per, C, seed, 1000 + rank * per, 1)
            assert p.tobytes() == whole[0][sl].tobytes() and np.array_equal(c, whole[1][sl])
    with pytest.raises(ValueError):
        dm.thin_host(base, M, C, seed, 0, 0)
    with pytest.raises(ValueError):
        dm.thin_host(base, M, C, seed, 0, C + 1)
    # the count draw sits at counter word 2 = 48, next to the RIR (16 + c) and noise (32) draws
    assert (dm._RIR_SLOT, dm._NOISE_SLOT, dm._COUNT_SLOT) == (16, 32, 48) and dm._RIR_SLOT + dm.MAX_C <= 32


@pytest.mark.parametrize("level_mode", [0, 1])
def test_mix_host_thinned_sources_are_exactly_zero(level_mode):
    import dynamic_mix as dm
    pool, off, spk = _corpus()
    M, C, T, seed = 16, 3, 700, 5
    base = dm.plan_host(off, spk, dm.eligible(off, T), M, C, T, seed=seed)
    plan, count = dm.thin_host(base, M, C, seed, 0, 1)
    assert count.min() < C
    out = dm.mix_host(pool, off, plan, T, level_mode=level_mode)
    assert not out["status"].any() and np.isfinite(out["mixture"]).all()
    for m in range(M):
        n = int(count[m])
        assert (np.abs(out["sources"][m, n:]) == 0).all() and (out["gains"][m, n:] == 0).all()
        assert (out["gains"][m, :n] > 0).all() and np.abs(out["sources"][m, :n]).max() > 0
        want = out["sources"][m, 0].copy()
        for c in range(1, n):
            want = want + out["sources"][m, c]
        assert np.array_equal(out["mixture"][m], want)              # the kept sources alone
    aug = dm.mix_aug_host(pool, off, plan, T, level_mode=level_mode)
    assert np.array_equal(aug["sources"], out["sources"]) and np.array_equal(aug["mixture"], out["mixture"])


# ---- the C ABI and the command-line surface --------------------------------------------------
def test_abi_validation(lib):
    import ctn_lib as L
    names = ("ctn_pitvar_workspace_bytes", "ctn_pitvar_forward", "ctn_pitvar_backward", "ctn_dmix_thin")
    for name in names:
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    ws = lambda **kw: lib.ctn_pitvar_workspace_bytes(ctypes.byref(L.PitVarDesc(**{**dict(
        M=3, C=4, T=300, mode=0, snr_max=30.0, inactive_snr_max=20.0), **kw})))
    assert ws() > 0 and ws(C=2) > 0 and ws(C=8, mode=1) > ws(C=2, mode=1)
    for bad in (dict(C=1), dict(C=9), dict(mode=2), dict(mode=-1), dict(snr_max=math.inf),
                dict(inactive_snr_max=math.nan), dict(M=0), dict(T=0)):
        assert ws(**bad) == 0, bad
        assert lib.ctn_last_error().decode()
    assert lib.ctn_pitvar_workspace_bytes(None) == 0
    # one slab of fp64 statistics (4C + C^2 + 1) per utterance and 2048-sample chunk, plus the fp64 maxima
    assert ws(M=1, C=8, T=2048) == 97 * 8 + 8 + 256 and ws(M=1, C=8, T=2049) == 2 * 97 * 8 + 8 + 256
    d = L.PitVarDesc(3, 4, 300, 0, 30.0, 20.0)
    assert lib.ctn_pitvar_forward(None, *([None] * 9), None, 0, None) == 1
    assert lib.ctn_pitvar_forward(ctypes.byref(d), *([None] * 9), None, 0, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_pitvar_backward(ctypes.byref(d), *([None] * 7), None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    for C in (1, 9):
        bad = L.PitVarDesc(3, C, 300, 0, 30.0, 20.0)
        assert lib.ctn_pitvar_forward(ctypes.byref(bad), *([None] * 9), None, 0, None) == 2
        assert f"C={C}" in lib.ctn_last_error().decode()
        assert lib.ctn_pitvar_backward(ctypes.byref(bad), *([None] * 7), None) == 2
    buf = ctypes.create_string_buffer(64)                            # never dereferenced: the workspace check is first
    p = ctypes.addressof(buf)
    assert lib.ctn_pitvar_forward(ctypes.byref(d), p, p, None, p, p, p, p, p, p, p, 64, None) == 3
    assert "workspace" in lib.ctn_last_error().decode()
    dd = L.DmixDesc(M=4, C=3, T=100, n_utts=5, n_elig=5, pool_dtype=0, level_mode=0, max_tries=4, level_lo_db=-1.0,
                    level_hi_db=1.0, peak=0.9, seed=1)
    for k in (0, 4):
        assert lib.ctn_dmix_thin(ctypes.byref(dd), k, 0, None, 0, p, p, None) == 1
        assert "min_speakers" in lib.ctn_last_error().decode()
    assert lib.ctn_dmix_thin(ctypes.byref(dd), 1, 0, None, 0, None, p, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_dmix_thin(None, 1, 0, None, 0, p, p, None) == 1


def test_train_flags_and_rejections():
    import train
    a = train.parser.parse_args([])
    assert (a.loss, a.var_loss, a.var_snr_max, a.var_inactive_snr_max, a.dm_min_speakers) == \
        ("pit", "snr", 30.0, 20.0, 0)
    train.check_var(a)
    a = train.parser.parse_args(["--loss", "pit_var", "--var_loss", "si_snr", "--C", "3", "--dm_min_speakers", "1",
                                 "--dynamic_mix", "1"])
    assert (a.loss, a.var_loss, a.dm_min_speakers) == ("pit_var", "si_snr", 1)
    train.check_var(a)
    train.check_var(train.parser.parse_args(["--loss", "mixit", "--C", "3", "--dm_min_speakers", "2",
                                             "--dynamic_mix", "1"]))
    train.check_var(train.parser.parse_args(["--loss", "pit", "--C", "3", "--dm_min_speakers", "3",
                                             "--dynamic_mix", "1"]))     # K = C: every slot speaks
    with pytest.raises(SystemExit) as ex:
        train.main(train.parser.parse_args(["--dm_min_speakers", "1", "--loss", "pit", "--dynamic_mix", "1"]))
    assert "silent" in str(ex.value) and "pit_var" in str(ex.value)
    with pytest.raises(SystemExit, match="--C"):
        train.main(train.parser.parse_args(["--dm_min_speakers", "3", "--loss", "pit_var", "--dynamic_mix", "1"]))
    with pytest.raises(SystemExit, match="--dynamic_mix"):
        train.main(train.parser.parse_args(["--dm_min_speakers", "1", "--loss", "pit_var"]))
    with pytest.raises(SystemExit, match="2 to 8"):
        train.main(train.parser.parse_args(["--loss", "pit_var", "--C", "1"]))
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--var_loss", "sdr"])


def test_evaluate_flag_defaults_off():
    import evaluate
    a = evaluate.parser.parse_args(["--model_path", "m", "--data_dir", "d"])
    assert (a.var_speakers, a.var_count_db, a.var_loss, a.var_snr_max, a.var_inactive_snr_max) == \
        (0, -20.0, "snr", 30.0, 20.0)
