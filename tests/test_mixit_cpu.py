"""MixIT without a GPU: the fp64 host restatement (mixit_criterion.mixit_host) on cases that
can be checked by hand, mom_pairs, the C-ABI's argument validation and the train.py flags."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mixit_cases as K


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


def test_host_exact_estimates_reach_the_ceiling():
    """Estimates equal to the planted sources, snr mode: R_n = 0 up to the fp32 rounding of
    x_n, so every row's score is 10 log10(1/tau) = snr_max (sources scaled by 32 so that EPS
    against tau X stays below 1e-9 dB), at the planted mask."""
    import mixit_criterion as mc
    for snr_max in (30.0, 20.0):
        mix, est, mask = K.planted(4, 3, 300, seed=1, a=1.0, b=0.0, off=0.0, scale=32.0)
        h = mc.mixit_host(mix, est, torch.tensor([300, 263, 226]), "snr", snr_max)
        assert h["scores"].shape == (3, 16)
        assert np.array_equal(h["assign"], mask.numpy())
        assert np.abs(h["max_snr"] - snr_max).max() < 1e-9
        assert abs(h["loss"] + snr_max) < 1e-9
        assert torch.equal(torch.from_numpy(h["remix"]), K.remix_fp32(est, mask, [300, 263, 226]))
        assert not h["remix"][1, :, 263:].any() and not h["remix"][2, :, 226:].any()


@pytest.mark.parametrize("mode", ["snr", "si_snr"])
def test_host_zero_channel_tie_goes_to_lower_p(mode):
    """An all-zero output changes no remixed sum: p and p ^ (1 << c) tie exactly and the
    first maximiser in ascending p has bit c = 0."""
    import mixit_criterion as mc
    mix, est, mask = K.planted(3, 2, 120, seed=2)
    est[:, 1] = 0.0
    h = mc.mixit_host(mix, est, torch.tensor([120, 77]), mode)
    assert np.array_equal(h["scores"][:, 0b000], h["scores"][:, 0b010])
    assert np.array_equal(h["assign"], (mask & ~2).numpy())
    est.zero_()                                              # all outputs zero: every p ties, p = 0 wins
    h = mc.mixit_host(mix, est, torch.tensor([120, 77]), mode)
    assert np.array_equal(h["assign"], [0, 0]) and np.isfinite(h["scores"]).all()


def test_host_matches_autograd_twin():
    """The numpy restatement and the torch fp64 twin are two statements of one definition."""
    import mixit_criterion as mc
    lens = torch.tensor([90, 61])
    for mode in ("snr", "si_snr"):
        mix, est, _ = K.planted(3, 2, 90, seed=3)
        h = mc.mixit_host(mix, est, lens, mode, 25.0)
        ms, loss, _ = K.twin(mix, est, lens, h["assign"], mode, 25.0, 1.0, [0.0, 0.0])
        assert np.abs(ms.numpy() - h["max_snr"]).max() < 1e-10 and abs(loss - h["loss"]) < 1e-10


def test_restated_coefficient_form_against_twin():
    """The backward's coefficient form (fp32 coefficients, fp64 evaluation, one rounding)
    reproduces the fp64 autograd gradient in both modes, within test_gpu_mixit.py's
    gradient bound (4 x the worst restated ratio over that file's cases, 2.05e-7)."""
    lens = torch.tensor([300, 263, 226])
    for mode in ("snr", "si_snr"):
        mix, est, mask = K.planted(4, 3, 300, seed=11)
        w = [0.3, -0.2, 0.5]
        _, _, g = K.twin(mix, est, lens, mask, mode, 30.0, 1.0, w)
        r = K.restated_grad(mix, est, lens, mask, mode, 30.0, 1.0, w)
        assert not r[1, :, 263:].any() and not g[2, :, 226:].any()
        assert K.row_ratio(r, g) <= 8.2e-7, mode


def test_mom_pairs_shapes_lengths_and_odd_batch():
    import mixit_criterion as mc
    mixture = torch.arange(5 * 7, dtype=torch.float32).reshape(5, 7)
    lengths = torch.tensor([7, 4, 3, 6, 5])
    mom, refs, lens = mc.mom_pairs(mixture, lengths)
    assert mom.shape == (2, 7) and refs.shape == (2, 2, 7) and lens.tolist() == [7, 6]
    assert torch.equal(refs[1, 0], mixture[2]) and torch.equal(refs[1, 1], mixture[3])
    assert torch.equal(mom, mixture[0:4:2] + mixture[1:4:2])
    assert refs.is_contiguous()
    mom, refs, lens = mc.mom_pairs(mixture[:4], lengths[:4])
    assert mom.shape == (2, 7) and lens.tolist() == [7, 6]


def test_abi_validation(lib):
    import ctn_lib as L
    assert L.ABI_VERSION == 13 and lib.ctn_abi_version() == 13      # added without a version bump
    for name in ("ctn_mixit_workspace_bytes", "ctn_mixit_forward", "ctn_mixit_backward"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    ws = lambda **kw: lib.ctn_mixit_workspace_bytes(ctypes.byref(L.MixitDesc(**{**dict(M=3, C=4, T=300, mode=0,
                                                                                      snr_max=30.0), **kw})))
    assert ws() > 0 and ws(C=2) > 0 and ws(C=8, mode=1) > ws(C=2, mode=1)
    for bad in (dict(C=1), dict(C=9), dict(mode=2), dict(mode=-1), dict(snr_max=math.inf), dict(snr_max=math.nan),
                dict(M=0), dict(T=0)):
        assert ws(**bad) == 0, bad
        assert lib.ctn_last_error().decode()
    assert lib.ctn_mixit_workspace_bytes(None) == 0
    # one slab of fp64 statistics per utterance and 2048-sample chunk, plus the fp64 maxima
    assert ws(M=1, C=8, T=2048) == 64 * 8 + 8 + 256 and ws(M=1, C=8, T=2049) == 2 * 64 * 8 + 8 + 256
    d = L.MixitDesc(3, 4, 300, 0, 30.0)
    assert lib.ctn_mixit_forward(None, *([None] * 8), None, 0, None) == 1
    assert lib.ctn_mixit_forward(ctypes.byref(d), *([None] * 8), None, 0, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_mixit_backward(ctypes.byref(d), *([None] * 8), None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_mixit_forward(ctypes.byref(L.MixitDesc(3, 9, 300, 0, 30.0)), *([None] * 8), None, 0, None) == 2
    assert "C=9" in lib.ctn_last_error().decode()
    buf = ctypes.create_string_buffer(64)                            # never dereferenced: the workspace check is first
    p = ctypes.addressof(buf)
    assert lib.ctn_mixit_forward(ctypes.byref(d), p, p, p, p, p, p, None, p, p, 64, None) == 3
    assert "workspace" in lib.ctn_last_error().decode()


def test_train_flags():
    import train
    a = train.parser.parse_args([])
    assert (a.loss, a.mixit_loss, a.mixit_snr_max, a.mixit_speakers) == ("pit", "snr", 30.0, 2)
    train.check_mixit(a)
    train.check_mixit(train.parser.parse_args(["--batch_size", "3", "--C", "1"]))    # pit: not MixIT's business
    a = train.parser.parse_args(["--loss", "mixit", "--mixit_loss", "si_snr", "--C", "4", "--batch_size", "8"])
    assert (a.loss, a.mixit_loss) == ("mixit", "si_snr")
    train.check_mixit(a)
    with pytest.raises(ValueError, match="batch_size 3"):
        train.main(train.parser.parse_args(["--loss", "mixit", "--batch_size", "3"]))
    with pytest.raises(ValueError, match="--C 1"):
        train.main(train.parser.parse_args(["--loss", "mixit", "--C", "1", "--batch_size", "4"]))
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--loss", "upit"])
    # rows of a loader batch: ceil(samples / segment) per utterance, or whole utterances
    assert train.minibatch_rows([[("a", 4000)], [("a1", 4000)], 8000, 4000]) == 1
    assert train.minibatch_rows([[("a", 9000), ("b", 4000)], [("a1", 9000), ("b1", 4000)], 8000, 4000]) == 4
    assert train.minibatch_rows([[("a", 9000), ("b", 4000)], [("a1", 9000), ("b1", 4000)], 8000, -1]) == 2


def test_evaluate_flag_defaults_off():
    import evaluate
    a = evaluate.parser.parse_args(["--model_path", "m", "--data_dir", "d"])
    assert (a.mixit_remix, a.mixit_loss, a.mixit_snr_max) == (0, "snr", 30.0)
