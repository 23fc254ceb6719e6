"""Device BSS Eval (ctn_bss_eval, ABI v13) checks that need no GPU: the entries are
exported, the workspace query follows the documented limits, arguments are validated before
any device access, and evaluate.py knows the opt-in flag."""
import ctypes
import os

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


def _ws(lib, *dims):
    import ctn_lib as L
    return lib.ctn_bss_workspace_bytes(ctypes.byref(L.BssDesc(*dims)))


def test_symbols_exported(lib):
    import ctn_lib as L
    assert L.ABI_VERSION == 13 and lib.ctn_abi_version() == 13
    for name in ("ctn_bss_workspace_bytes", "ctn_bss_eval"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert [f[0] for f in L.BssDesc._fields_] == ["M", "C", "E", "T", "flen"]
    assert ctypes.sizeof(L.BssDesc) == 20


def test_workspace_bytes(lib):
    two = _ws(lib, 2, 2, 3, 700, 16)
    assert two > 0
    assert _ws(lib, 4, 2, 3, 700, 16) > two > _ws(lib, 1, 2, 3, 700, 16)
    assert _ws(lib, 1, 8, 9, 1100, 512) > 0              # C * flen = 4096: the limit itself
    assert _ws(lib, 1, 9, 10, 1100, 512) == 0            # C * flen = 4608 > 4096
    assert _ws(lib, 1, 1, 1, 8192, 4097) == 0
    assert _ws(lib, 2, 2, 3, 15, 16) == 0                # T < flen
    for bad in ((0, 2, 3, 700, 16), (2, 0, 3, 700, 16), (2, 2, 0, 700, 16), (2, 2, 3, 700, 0)):
        assert _ws(lib, *bad) == 0
    assert lib.ctn_bss_workspace_bytes(None) == 0


def test_eval_validates_before_the_device(lib):
    import ctn_lib as L
    d = L.BssDesc(2, 2, 3, 700, 16)
    assert lib.ctn_bss_eval(ctypes.byref(d), None, None, None, None, None, None, 0, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_bss_eval(None, None, None, None, None, None, None, 0, None) == 1
    assert lib.ctn_last_error().decode()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    for bad in ((0, 2, 3, 700, 16), (2, 2, 3, 700, 0), (2, 2, 3, 15, 16)):
        assert lib.ctn_bss_eval(ctypes.byref(L.BssDesc(*bad)), p, p, p, p, p, p, 64, None) == 1
    assert "shorter than the 16-tap" in lib.ctn_last_error().decode()
    assert lib.ctn_bss_eval(ctypes.byref(L.BssDesc(1, 9, 10, 1100, 512)), p, p, p, p, p, p, 64, None) == 2
    assert "4096" in lib.ctn_last_error().decode()
    assert lib.ctn_bss_eval(ctypes.byref(d), p, p, p, p, p, None, 0, None) == 3      # no workspace
    assert lib.ctn_bss_eval(ctypes.byref(d), p, p, p, p, p, p, 64, None) == 3        # short workspace
    assert "workspace" in lib.ctn_last_error().decode()


def test_evaluate_parser_has_sdr_device():
    import evaluate
    base = ["--model_path", "m.pth.tar", "--data_dir", "d"]
    assert evaluate.parser.parse_args(base).sdr_device == 0
    assert evaluate.parser.parse_args(base + ["--cal_sdr", "1", "--sdr_device", "1"]).sdr_device == 1


def test_host_side_batch_checks_need_no_library():
    """The ValueErrors of bss_eval_sources, raised for a padded batch before any library call."""
    import torch

    import bss_eval
    x = torch.ones(2, 2, 64)
    with pytest.raises(ValueError, match="shape mismatch"):
        bss_eval._check_batch(x, torch.ones(2, 3, 64), None, 16)
    with pytest.raises(ValueError, match="shorter than the 16-tap"):
        bss_eval._check_batch(x, x, torch.tensor([64, 15]), 16)
    z = x.clone()
    z[1, 0, :40] = 0                                     # zero inside its length of 40 only
    with pytest.raises(ValueError, match="all zeros"):
        bss_eval._check_batch(z, z, torch.tensor([64, 40]), 16)
    assert bss_eval._check_batch(z, z, torch.tensor([64, 41]), 16)[1] == [64, 41]
    assert bss_eval._on_host([0, 1, 0], [64, 64, 16], 2, 16) == [False, True, True]
