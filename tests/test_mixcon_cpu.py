"""Mixture consistency without a GPU: the fp64 host restatement
(mixture_consistency.mixture_consistency_host) on cases that can be checked by hand, its
backward formula against torch fp64 autograd of the definition, the C-ABI's argument
validation, the package keys, the train.py flag and the streamer's rejection."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mixcon_cases as K


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


def test_abi_validation(lib):
    import ctn_lib as L
    assert L.ABI_VERSION == 13 and lib.ctn_abi_version() == 13      # added without a version bump
    for name in ("ctn_mixcon_workspace_bytes", "ctn_mixcon_forward", "ctn_mixcon_backward"):
        assert name in L.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert L.MixconDesc._fields_ == [(n, ctypes.c_int32) for n in ("M", "C", "T", "mode")]
    ws = lambda **kw: lib.ctn_mixcon_workspace_bytes(ctypes.byref(L.MixconDesc(**{**dict(M=3, C=4, T=300, mode=1),
                                                                                   **kw})))
    assert ws() > 0 and ws(C=2, mode=0) > 0 and ws(C=16) > ws(C=2)
    for bad in (dict(C=1), dict(C=17), dict(M=0), dict(T=0), dict(mode=2), dict(mode=-1)):
        assert ws(**bad) == 0, bad
        assert lib.ctn_last_error().decode()
    assert lib.ctn_mixcon_workspace_bytes(None) == 0
    # C fp64 partials per utterance and 2048-sample chunk (64 chunks at most), C backward coefficients
    assert ws(M=1, C=8, T=2048) == (8 + 8) * 8 + 256 and ws(M=1, C=8, T=2049) == (16 + 8) * 8 + 256
    assert ws(M=2, C=2, T=131073) == ws(M=2, C=2, T=1 << 20) == 2 * (64 * 2 + 2) * 8 + 256
    d = L.MixconDesc(3, 4, 300, 1)
    assert lib.ctn_mixcon_forward(None, *([None] * 5), None, 0, None) == 1
    assert lib.ctn_mixcon_forward(ctypes.byref(d), *([None] * 5), None, 0, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_mixcon_backward(ctypes.byref(d), *([None] * 7), None, 0, None) == 1
    assert "null pointer" in lib.ctn_last_error().decode()
    assert lib.ctn_mixcon_forward(ctypes.byref(L.MixconDesc(3, 17, 300, 1)), *([None] * 5), None, 0, None) == 2
    assert "C=17" in lib.ctn_last_error().decode()
    buf = ctypes.create_string_buffer(64)                            # never dereferenced: the checks come first
    p, q = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    assert lib.ctn_mixcon_forward(ctypes.byref(d), p, p, None, q, p, p, 64, None) == 3
    assert "workspace" in lib.ctn_last_error().decode()
    assert lib.ctn_mixcon_forward(ctypes.byref(d), p, p, None, q, p, None, 1 << 20, None) == 3
    assert lib.ctn_mixcon_backward(ctypes.byref(d), p, p, None, p, p, q, None, p, 64, None) == 3
    assert lib.ctn_mixcon_forward(ctypes.byref(d), p, p, None, p, p, p, 1 << 20, None) == 1       # in place
    assert "in place" in lib.ctn_last_error().decode()
    du = L.MixconDesc(3, 4, 300, 0)                                  # uniform needs no coef, power does
    assert lib.ctn_mixcon_forward(ctypes.byref(du), p, p, None, q, None, p, 64, None) == 3
    assert lib.ctn_mixcon_forward(ctypes.byref(d), p, p, None, q, None, p, 1 << 20, None) == 1


@pytest.mark.parametrize("mode", K.MODES)
def test_host_forward_sums_to_the_mixture(mode):
    import mixture_consistency as mc
    x, s, _ = K.make(3, 5, 400, seed=1)
    lens = torch.tensor([400, 0, 123])
    h = mc.mixture_consistency_host(x, s, lens, mode)
    for m, n in enumerate(lens.tolist()):
        top = float(s[m].abs().max())
        assert np.abs(h["out"][m, :, :n].sum(0) - x[m, :n].double().numpy()).max(initial=0.0) <= 1e-13 * top
        assert np.array_equal(h["out"][m, :, n:], s[m, :, n:].double().numpy())
    assert np.abs(h["w"].sum(1) - 1.0).max() <= 1e-15
    if mode == "uniform":
        assert np.array_equal(h["w"], np.full((3, 5), 0.2))
    full = mc.mixture_consistency_host(x, s, None, mode)             # no lengths: every sample
    assert np.abs(full["out"].sum(1) - x.double().numpy()).max() <= 1e-13 * float(s.abs().max())
    with pytest.raises(ValueError):
        mc.mixture_consistency_host(x, s, lens, "energy")


def test_host_power_weights():
    """1/C on all-zero outputs (and on an utterance of length 0); on outputs of planted
    energy e_c the weights are (e_c + EPS) / (sum e + C EPS)."""
    import mixture_consistency as mc
    x, s, _ = K.make(2, 4, 64, seed=2)
    h = mc.mixture_consistency_host(x, torch.zeros_like(s), None, "power")
    assert np.array_equal(h["w"], np.full((2, 4), 0.25))
    assert np.abs(h["out"] - x.double().numpy()[:, None, :] / 4).max() <= 1e-16
    assert np.array_equal(mc.mixture_consistency_host(x, s, torch.tensor([0, 0]), "power")["w"], np.full((2, 4), 0.25))
    amp = torch.tensor([1.0, 2.0, 0.0, 0.5])
    sign = torch.where(torch.arange(64) % 2 == 0, 1.0, -1.0)
    planted = (amp[:, None] * sign[None, :]).expand(2, 4, 64).contiguous()      # energy 64 amp^2, exact in fp64
    lens = torch.tensor([64, 16])
    h = mc.mixture_consistency_host(x, planted, lens, "power")
    for m, n in enumerate(lens.tolist()):
        e = n * amp.double().numpy() ** 2
        assert np.abs(h["w"][m] - (e + 1e-8) / (e.sum() + 4e-8)).max() <= 1e-15
        assert h["D"][m] == e.sum() + 4e-8
    assert h["w"][0, 2] < 1e-9 and abs(h["w"].sum(1) - 1.0).max() <= 1e-15


@pytest.mark.parametrize("mode", K.MODES)
@pytest.mark.parametrize("C", [2, 3, 8])
def test_backward_formula_against_autograd(mode, C):
    """The restated backward formula against torch fp64 autograd of the definition, lengths 0,
    1 and T, a random upstream gradient: both sides are fp64, only the summation order differs."""
    import mixture_consistency as mc
    T = 257
    x, s, g = K.make(3, C, T, seed=30 + C)
    lens = torch.tensor([0, 1, T])
    out, gs, gx = K.twin(x, s, g, lens, mode)
    h = mc.mixture_consistency_host(x, s, lens, mode, grad_out=g)
    assert np.abs(h["out"] - out.numpy()).max() <= 1e-12 * float(s.abs().max())
    assert K.row_ratio(torch.from_numpy(h["g_est"]), gs) <= 1e-12
    assert K.row_ratio(torch.from_numpy(h["g_mixture"]), gx) <= 1e-12
    assert np.array_equal(h["g_est"][0], g[0].double().numpy()) and not h["g_mixture"][0].any()
    assert np.array_equal(h["g_est"][1, :, 1:], g[1, :, 1:].double().numpy()) and not h["g_mixture"][1, 1:].any()


def test_restated_device_evaluation_against_autograd():
    """mixcon_cases.restated (the device's evaluation: chunk-ordered fp64 sums, one rounding)
    within a quarter of test_gpu_mixcon.py's gradient bound on a two-chunk case."""
    from test_gpu_mixcon import GRAD_BOUND
    for mode in K.MODES:
        x, s, g = K.make(3, 3, 2049, seed=40)
        lens = K.lengths3(2049, 3)
        _, gs, gx = K.twin(x, s, g, lens, mode)
        r = K.restated(x, s, g, lens, mode)
        assert K.row_ratio(r["g_est"], gs) <= GRAD_BOUND / 4 and K.row_ratio(r["g_mixture"], gx) <= GRAD_BOUND / 4


# the reference's package keys (src/conv_tasnet.py:78-94) as ConvTasNet.serialize writes them today
PACKAGE_KEYS = {'N', 'L', 'B', 'H', 'P', 'X', 'R', 'C', 'norm_type', 'causal', 'mask_nonlinear', 'state_dict',
                'optim_dict', 'epoch', 'tr_loss', 'cv_loss'}


def test_package_keys_and_round_trip():
    import conv_tasnet as ct
    model = ct.ConvTasNet(16, 8, 16, 32, 3, 2, 1, 3)
    assert model.mixture_consistency == 'none'
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    pkg = ct.ConvTasNet.serialize(model, opt, 1, tr_loss=torch.zeros(1), cv_loss=torch.zeros(1))
    assert set(pkg) == PACKAGE_KEYS
    assert set(ct.ConvTasNet.serialize(model, opt, 1)) == PACKAGE_KEYS - {'tr_loss', 'cv_loss'}
    assert ct.ConvTasNet.load_model_from_package(pkg).mixture_consistency == 'none'    # no key: none
    on = ct.ConvTasNet(16, 8, 16, 32, 3, 2, 1, 3, mixture_consistency='power')
    assert [n for n, _ in on.named_parameters()] == [n for n, _ in model.named_parameters()]
    assert list(on.state_dict()) == list(model.state_dict())          # no parameters, no buffers
    pkg = ct.ConvTasNet.serialize(on, opt, 1, tr_loss=torch.zeros(1), cv_loss=torch.zeros(1))
    assert set(pkg) == PACKAGE_KEYS | {'mixture_consistency'} and pkg['mixture_consistency'] == 'power'
    back = ct.ConvTasNet.load_model_from_package(pkg)
    assert back.mixture_consistency == 'power'
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), on.state_dict().values()))
    with pytest.raises(ValueError, match="mixture_consistency"):
        ct.ConvTasNet(16, 8, 16, 32, 3, 2, 1, 3, mixture_consistency='energy')
    with pytest.raises(ValueError, match="C=1"):
        ct.ConvTasNet(16, 8, 16, 32, 3, 2, 1, 1, mixture_consistency='uniform')


def test_train_flag():
    import train
    a = train.parser.parse_args([])
    assert a.mixture_consistency == "none"
    train.check_mixture_consistency(a)
    a = train.parser.parse_args(["--mixture_consistency", "power", "--loss", "mixit", "--C", "4"])
    assert a.mixture_consistency == "power"
    train.check_mixture_consistency(a)
    with pytest.raises(SystemExit):
        train.parser.parse_args(["--mixture_consistency", "energy"])
    with pytest.raises(ValueError, match="--C 1"):
        train.main(train.parser.parse_args(["--mixture_consistency", "uniform", "--C", "1"]))


@pytest.mark.parametrize("mode", K.MODES)
def test_streaming_rejects_a_consistent_model(mode):
    """At construction, where the streamer's other rejections happen: no device call."""
    import conv_tasnet as ct
    from streaming import StreamingSeparator
    model = ct.ConvTasNet(16, 8, 16, 32, 3, 2, 1, 2, norm_type="cLN", causal=True, mixture_consistency=mode).eval()
    with pytest.raises(ValueError, match="mixture consistency"):
        StreamingSeparator(model)


def test_device_call_needs_a_device():
    import ctn_lib as L
    import mixture_consistency as mc
    x, s, _ = K.make(1, 2, 16, seed=3)
    with pytest.raises(L.CtnLibraryError):
        mc.mixture_consistency(x, s)                                  # host tensors: no fallback
    with pytest.raises(ValueError):
        mc.mixture_consistency(x, s, None, "none")
