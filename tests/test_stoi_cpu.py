"""STOI / ESTOI checks that need no GPU: the host restatement (stoi.py) against the defining
properties of the metric — band table, resampling filter and index formula, identity,
monotonicity in the SNR, scale invariance, the 30-frame edge — and the C ABI of the device
path (ctn_stoi_*): exported symbols, table and workspace queries, argument validation before
any device access, the evaluate.py flag and the benchmark's command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

LO = [7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174]
HI = [9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219]


def _speech(T, seed, c=0):
    import synthetic
    return synthetic.speech_like(1, 2, T, seed)[1][0, c].numpy().astype(np.float64)


def test_band_table():
    import stoi
    assert stoi.thirdoct(10000, 512, 15, 150) == (LO, HI)
    assert (stoi.BAND_LO, stoi.BAND_HI) == (LO, HI)


def test_resampling_filter_half_lengths():
    import stoi
    assert stoi.ratio(8000) == (5, 4) and stoi.ratio(16000) == (5, 8) and stoi.ratio(10000) == (1, 1)
    for (up, down), Hl in (((5, 4), 182), ((5, 8), 290)):
        win, got = stoi.resample_filter(up, down)
        assert got == Hl and win.size == 2 * Hl + 1
        assert abs(win.sum() - 1.0) < 1e-15
        np.testing.assert_array_equal(win, win[::-1])


@pytest.mark.parametrize("fs,n", [(8000, 701), (16000, 1203)])
def test_index_formula_equals_resample_poly(fs, n):
    import stoi
    x = _speech(n, 3)
    up, down = stoi.ratio(fs)
    direct = stoi.resample_direct(x, up, down)
    assert direct.size == -(-n * up // down)
    assert np.abs(direct - stoi.resample(x, fs)).max() == 0.0


def test_identity_is_one():
    import stoi
    x = _speech(32000, 0)
    r = stoi.stoi_details(x, x, 8000)
    assert abs(r.stoi - 1.0) <= 1e-9 and abs(r.estoi - 1.0) <= 1e-9
    assert stoi.stoi(x, x, 8000) == r.stoi and stoi.stoi(x, x, 8000, extended=True) == r.estoi


def test_scores_fall_with_the_snr_and_ignore_the_scale():
    import stoi
    x = _speech(32000, 0, c=1)
    noise = np.random.default_rng(1234).standard_normal(x.size) * x.std()
    got = []
    for snr in (100, 5, -5):
        y = x + noise * 10 ** (-snr / 20)
        r = stoi.stoi_details(x, y, 8000)
        got.append((r.stoi, r.estoi))
        for g in (0.01, 100.0):
            s = stoi.stoi_details(x, g * y, 8000)
            assert abs(s.stoi - r.stoi) <= 1e-12 and abs(s.estoi - r.estoi) <= 1e-12
    print(got)
    for k in (0, 1):
        assert 1.0 >= got[0][k] > got[1][k] > got[2][k] > 0.0


def test_thirty_frame_edge():
    import stoi
    x = _speech(4000, 5)
    r = stoi.stoi_details(x[:3968], x[:3968], 10000)
    assert r.kept == 30 and list(r.idx) == list(range(30)) and abs(r.stoi - 1.0) <= 1e-9
    r = stoi.stoi_details(x[:3967], x[:3967], 10000)
    assert r.kept == 29 and r.stoi == 1e-5 and r.estoi == 1e-5
    assert stoi.stoi(x[:3967], x[:3967], 10000) == 1e-5
    assert stoi.stoi_details(x[:3174], x[:3174], 8000).kept == 30
    r = stoi.stoi_details(x[:3173], x[:3173], 8000)
    assert r.kept == 29 and r.stoi == 1e-5
    assert stoi.stoi_details(x[:100], x[:100], 8000).kept == 0


def test_silent_frames_are_dropped_and_margin_reported():
    import stoi
    x = _speech(16000, 6)
    full = stoi.stoi_details(x, x, 10000)
    x[4000:8000] *= 1e-4
    r = stoi.stoi_details(x, x, 10000)
    assert 30 <= r.kept < full.kept and r.margin > 0
    assert not set(range(33, 60)) & set(r.idx.tolist())          # frames wholly inside the pause
    with pytest.raises(ValueError):
        stoi.stoi(x, x[:-1], 10000)


def test_device_ratio_limits():
    import stoi
    assert stoi.device_ratio(8000) == (5, 4, 182) and stoi.device_ratio(10000) == (1, 1, 0)
    assert stoi.device_ratio(48000) == (5, 24, stoi.resample_filter(5, 24)[1])
    with pytest.raises(ValueError, match="44100"):
        stoi.device_ratio(44100)
    t = stoi.table(16000)
    assert t.size == 256 + 512 + 2 * 290 + 1 and t.dtype == np.float64
    np.testing.assert_array_equal(t[:256], np.hanning(258)[1:-1])
    assert t[256] == 1.0 and t[257] == 0.0 and abs(t[256 + 2 * 128]) < 1e-15 and t[256 + 2 * 128 + 1] == -1.0
    assert abs(t[768:].sum() - 5.0) < 1e-12
    assert stoi.table(10000).size == 768


# ----------------------------------------------------------------------------
# C ABI
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


GOOD = (2, 2, 3, 8000, 5, 4, 182)
BAD = (
    (0, 2, 3, 8000, 5, 4, 182), (2, 0, 3, 8000, 5, 4, 182), (2, 2, 0, 8000, 5, 4, 182), (2, 2, 3, 0, 5, 4, 182),
    (65536, 2, 3, 8000, 5, 4, 182), (2, 2, 65536, 8000, 5, 4, 182), (2, 17, 3, 8000, 5, 4, 182),
    (2, 2, 3, 8000, 0, 4, 182), (2, 2, 3, 8000, 5, 0, 182), (2, 2, 3, 8000, 65, 4, 182), (2, 2, 3, 8000, 5, 67, 182),
    (2, 2, 3, 8000, 10, 8, 182),                                     # not reduced
    (2, 2, 3, 8000, 5, 4, 0), (2, 2, 3, 8000, 5, 4, 4097),
    (2, 2, 3, 2 ** 31 - 1, 5, 4, 182),                               # 2^31 resampled samples and more
)


def test_symbols_exported(lib):
    import ctn_lib as L
    assert L.ABI_VERSION == 13 and lib.ctn_abi_version() == 13
    for name in ("ctn_stoi_table_doubles", "ctn_stoi_workspace_bytes", "ctn_stoi_eval"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert [f[0] for f in L.StoiDesc._fields_] == ["M", "C", "E", "T", "up", "down", "Hl"]
    assert ctypes.sizeof(L.StoiDesc) == 28


def test_table_doubles(lib):
    import ctn_lib as L
    import stoi
    for fs in (8000, 16000, 10000, 48000):
        up, down, Hl = stoi.device_ratio(fs)
        want = 256 + 512 + (0 if up == down else 2 * Hl + 1)
        assert lib.ctn_stoi_table_doubles(ctypes.byref(L.StoiDesc(1, 1, 1, 100, up, down, Hl))) == want
        assert stoi.table(fs).size == want
    assert lib.ctn_stoi_table_doubles(ctypes.byref(L.StoiDesc(1, 1, 1, 100, 1, 1, 777))) == 768   # Hl ignored at 1/1
    assert lib.ctn_stoi_table_doubles(None) == 0
    for bad in BAD:
        assert lib.ctn_stoi_table_doubles(ctypes.byref(L.StoiDesc(*bad))) == 0, bad


def test_workspace_bytes(lib):
    import ctn_lib as L

    def ws(*dims):
        return lib.ctn_stoi_workspace_bytes(ctypes.byref(L.StoiDesc(*dims)))
    two = ws(*GOOD)
    assert two > 0 and ws(4, *GOOD[1:]) > two > ws(1, *GOOD[1:])
    assert two >= 2 * (2 + 3) * 10000 * 8                        # at least the resampled rows
    assert ws(65535, 16, 1, 1, 64, 63, 4096) > 0                 # every limit itself
    assert ws(1, 1, 1, 100, 1, 1, 0) > 0                         # shorter than one frame: still a call
    assert lib.ctn_stoi_workspace_bytes(None) == 0
    for bad in BAD:
        assert ws(*bad) == 0, bad


def test_eval_validates_before_the_device(lib):
    import ctn_lib as L
    d = L.StoiDesc(*GOOD)
    nul = (None,) * 7
    assert lib.ctn_stoi_eval(ctypes.byref(d), *nul, None, 0, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_stoi_eval(None, *nul, None, 0, None) == 1
    assert "descriptor" in lib.ctn_last_error().decode()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ptrs = (p,) * 7
    for k in range(7):                                            # every single null pointer
        one = tuple(None if i == k else p for i in range(7))
        assert lib.ctn_stoi_eval(ctypes.byref(d), *one, p, 64, None) == 1
    for bad in BAD:
        rc = lib.ctn_stoi_eval(ctypes.byref(L.StoiDesc(*bad)), *ptrs, p, 64, None)
        assert rc in (1, 2) and lib.ctn_last_error().decode(), bad
    assert lib.ctn_stoi_eval(ctypes.byref(L.StoiDesc(2, 17, 3, 8000, 5, 4, 182)), *ptrs, p, 64, None) == 2
    assert "16" in lib.ctn_last_error().decode()
    assert lib.ctn_stoi_eval(ctypes.byref(L.StoiDesc(2, 2, 3, 8000, 10, 8, 182)), *ptrs, p, 64, None) == 1
    assert "reduced" in lib.ctn_last_error().decode()
    assert lib.ctn_stoi_eval(ctypes.byref(d), *ptrs, None, 0, None) == 3          # no workspace
    assert lib.ctn_stoi_eval(ctypes.byref(d), *ptrs, p, 64, None) == 3            # short workspace
    assert "workspace" in lib.ctn_last_error().decode()


def test_evaluate_parser_has_cal_stoi():
    import evaluate
    base = ["--model_path", "m.pth.tar", "--data_dir", "d"]
    assert evaluate.parser.parse_args(base).cal_stoi == 0
    assert evaluate.parser.parse_args(base + ["--cal_stoi", "1"]).cal_stoi == 1


def test_evaluator_rejects_an_unsupported_rate():
    import evaluate
    args = evaluate.parser.parse_args(["--model_path", "m.pth.tar", "--data_dir", "d", "--cal_stoi", "1",
                                       "--sample_rate", "44100"])
    with pytest.raises(SystemExit, match="44100"):
        evaluate.Evaluator(args)


def test_bench_stoi_help_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_stoi.py"), "--help"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "--M" in out.stdout
