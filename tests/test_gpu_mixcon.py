"""Mixture-consistency kernels (csrc/ctn_mixcon.hip) against fp64 references on the host.

Every case of mixcon_cases.py is checked the same way (``_check``):

* forward against ``mixture_consistency.mixture_consistency_host`` (fp64, unrounded), per
  sample |dev - ref| <= 2^-23 |ref| + 2^-40 max(|x[t]|, max_c |s_c[t]|): one fp32 rounding of
  an fp64 value plus fp64 evaluation noise under cancellation;
* bit-equal pass-through at t >= length; sum_c y_c = x within C 2^-23 max_c |y_c| at t < length;
* ``weights`` within 1e-12 of the host's;
* backward against the fp64 torch autograd twin of the definition (mixcon_cases.twin), per
  row max_t |dev - ref| <= GRAD_BOUND max_t |ref| for dL/ds and dL/dx; dL/ds = g bit for bit
  and dL/dx = 0 at t >= length.

GRAD_BOUND: the device evaluates g_k - G + s_k k_k in fp64 and rounds once.  Restated on the
host (mixcon_cases.restated: the same fp64 sums folded in the device's chunk order) against
the twin, the worst row ratio over all cases of this file is 5.85e-8 (T = 1, C = 3, uniform; a row's
largest entry rounded the worst way, 2^-24 = 5.96e-8, is the ceiling); the bound is 4x that,
2.34e-7.  Measured on the MI355X: 5.85e-8, every case agreeing with its restated figure to
three digits.
"""
import io
import os
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import mixcon_cases as K

pytestmark = pytest.mark.gpu

RESTATED = 5.85e-8
GRAD_BOUND = 4 * RESTATED


def _device(x, s, g, lens, mode, want_gx=True):
    import mixture_consistency as mc
    xs, e = x.cuda().requires_grad_(want_gx), s.cuda().requires_grad_(True)
    before = e.detach().clone()
    ld = None if lens is None else lens.cuda()
    y = mc.mixture_consistency(xs, e, ld, mode)
    y.backward(g.cuda())
    assert torch.equal(e.detach(), before), "est was modified"
    assert y.shape == s.shape and y.dtype == torch.float32 and y.data_ptr() != e.data_ptr()
    w = mc.weights(xs.detach(), e.detach(), ld, mode)
    assert w.dtype == torch.float64 and w.shape == s.shape[:2]
    return y.detach().cpu(), e.grad.cpu(), xs.grad.cpu() if want_gx else None, w.cpu()


def _check(name, x, s, g, lens, mode):
    """The checks of the module docstring -> the measured gradient row ratio."""
    import mixture_consistency as mc
    M, C, T = s.shape
    y, gs, gx, w = _device(x, s, g, lens, mode)
    h = mc.mixture_consistency_host(x, s, lens, mode)
    ref = torch.from_numpy(h["out"])
    scale = torch.maximum(x.double().abs().unsqueeze(1), s.double().abs().amax(1, keepdim=True))
    excess = (y.double() - ref).abs() - (2.0 ** -23 * ref.abs() + 2.0 ** -40 * scale)
    assert float(excess.max()) <= 0.0, (name, float(excess.max()))
    assert float((w - torch.from_numpy(h["w"])).abs().max()) <= 1e-12, name
    for m, n in enumerate(K.lens_list(lens, M, T)):
        assert torch.equal(y[m, :, n:], s[m, :, n:]), (name, m)
        assert torch.equal(gs[m, :, n:], g[m, :, n:]) and not gx[m, n:].any(), (name, m)
        gap = (y[m, :, :n].double().sum(0) - x[m, :n].double()).abs() - C * 2.0 ** -23 * y[m, :, :n].double().abs().amax(0)
        assert n == 0 or float(gap.max()) <= 0.0, (name, m, float(gap.max()))
    _, gs_ref, gx_ref = K.twin(x, s, g, lens, mode)
    ratio = max(K.row_ratio(gs, gs_ref), K.row_ratio(gx, gx_ref))
    print(f"{name}: gradient row ratio {ratio:.3e} (bound {GRAD_BOUND:.2e})")
    assert ratio <= GRAD_BOUND, (name, ratio)
    return ratio


@pytest.mark.parametrize("T", K.GRID_T)
def test_grid(T):
    """C = 2, 3, 8, 16; M = 1 (no lengths) and 3 (lengths 0 or 1, n < T, T); both modes."""
    for case in K.grid_cases(T):
        _check(*case)


def test_chunk_clamp():
    """T = 131073 = 64 * 2048 + 1: past the 64-chunk cap, and past 256 element-wise workgroups."""
    for case in K.clamp_cases():
        _check(*case)


def test_special_cases():
    """r = 0 exactly, all-zero outputs, one output 1e4 times louder than the rest."""
    import mixture_consistency as mc
    for case in K.special_cases():
        name, x, s, g, lens, mode = case
        _check(*case)
        if name.startswith("r=0"):
            assert torch.equal(mc.mixture_consistency(x.cuda(), s.cuda(), lens.cuda(), mode).cpu(), s)
        if name.startswith("zero outputs"):
            assert torch.equal(mc.weights(x.cuda(), s.cuda(), lens.cuda(), mode).cpu(), torch.full((4, 4), 0.25,
                                                                                                  dtype=torch.float64))
        if name == "loud output power":
            assert float(mc.weights(x.cuda(), s.cuda(), lens.cuda(), mode)[3, 1]) > 1.0 - 1e-6


def test_deterministic_and_mixture_gradient_optional():
    """Two runs give the same bits; without a gradient for the mixture (null pointer) dL/ds is
    the same and no mixture gradient exists."""
    x, s, g = K.make(3, 8, 2049, seed=5)
    lens = K.lengths3(2049, 8)
    for mode in K.MODES:
        a, b = _device(x, s, g, lens, mode), _device(x, s, g, lens, mode)
        for u, v in zip(a, b):
            assert torch.equal(u, v)
        c = _device(x, s, g, lens, mode, want_gx=False)
        assert c[2] is None and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])


def test_backward_entry_leaves_a_null_mixture_gradient_alone():
    """ctn_mixcon_backward with g_mixture = NULL against the same call with a buffer: the same
    dL/ds, and nothing but g_est is written (a guard buffer placed where dL/dx would go stays)."""
    import ctypes
    import ctn_lib as L
    lib = L.load()
    x, s, g = (t.cuda() for t in K.make(2, 3, 301, seed=6))
    d = L.MixconDesc(2, 3, 301, L.MIXCON_UNIFORM)
    nb = lib.ctn_mixcon_workspace_bytes(ctypes.byref(d))
    ws = L.workspace(nb, x.device)
    ge1, ge2 = torch.empty_like(s), torch.empty_like(s)
    gx = torch.full_like(x, 7.0)
    st = L.stream_handle(x.device)
    L.check(lib.ctn_mixcon_backward(ctypes.byref(d), None, None, None, None, g.data_ptr(), ge1.data_ptr(), None,
                                    ws.data_ptr(), nb, st), "ctn_mixcon_backward")
    torch.cuda.synchronize()
    assert bool((gx == 7.0).all())
    L.check(lib.ctn_mixcon_backward(ctypes.byref(d), None, None, None, None, g.data_ptr(), ge2.data_ptr(),
                                    gx.data_ptr(), ws.data_ptr(), nb, st), "ctn_mixcon_backward")
    torch.cuda.synchronize()
    assert torch.equal(ge1, ge2) and not bool((gx == 7.0).any())


def test_capturable_into_a_graph():
    """Neither call synchronises: forward and backward are captured into a graph whose replay
    on fresh inputs gives the eager call's bits."""
    import mixture_consistency as mc
    x0, s0, g0 = K.make(3, 4, 2049, seed=8)
    lens = K.lengths3(2049, 4).cuda()
    x, e = torch.zeros_like(x0).cuda(), torch.zeros_like(s0).cuda().requires_grad_(True)
    g = g0.cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up outside the capture
        torch.autograd.grad(mc.mixture_consistency(x, e, lens, "power"), e, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = mc.mixture_consistency(x, e, lens, "power")
        grad, = torch.autograd.grad(y, e, g)
    x.copy_(x0)
    with torch.no_grad():
        e.copy_(s0)
    graph.replay()
    torch.cuda.synchronize()
    e2 = s0.cuda().requires_grad_(True)
    want = mc.mixture_consistency(x0.cuda(), e2, lens, "power")
    assert torch.equal(y, want) and torch.equal(grad, torch.autograd.grad(want, e2, g)[0])


def test_bad_arguments_raise():
    import ctn_lib as L
    import mixture_consistency as mc
    x, s, _ = K.make(2, 3, 50, seed=1)
    with pytest.raises(ValueError):
        mc.mixture_consistency(x.cuda(), s.cuda(), None, "energy")
    with pytest.raises(ValueError):
        mc.mixture_consistency(x[:, :49].cuda(), s.cuda())
    with pytest.raises(ValueError):
        mc.mixture_consistency(x.cuda(), s.cuda(), torch.tensor([50]))
    with pytest.raises(L.CtnLibraryError):
        mc.mixture_consistency(x.cuda(), s[:, :1].contiguous().cuda())          # C = 1
    with pytest.raises(L.CtnLibraryError):
        mc.mixture_consistency(x.cuda(), s.cuda().transpose(1, 2).contiguous().transpose(1, 2))


# ---- model level: N = 32, L = 16, B = 32, H = 64, P = 3, X = 2, R = 1, C = 4, gLN, T = 4000 ----------
CFG = (32, 16, 32, 64, 3, 2, 1, 4)


def _model(mode=None, seed=0):
    import conv_tasnet as ct
    torch.manual_seed(seed)
    kw = {} if mode is None else dict(mixture_consistency=mode)
    return ct.ConvTasNet(*CFG, **kw).cuda().eval()


def _sums_to(est, mix, what):
    """sum_c est_c = mix per sample within C 2^-23 max_c |est_c| (the forward bound above)."""
    C = est.size(1)
    gap = (est.double().sum(1) - mix.double()).abs() - C * 2.0 ** -23 * est.double().abs().amax(1)
    assert float(gap.max()) <= 0.0, (what, float(gap.max()))


def test_model_outputs_sum_to_the_input():
    import synthetic
    mix, _ = synthetic.speech_like(3, 2, 4000, 11)
    mix = mix.cuda()
    lens = torch.tensor([4000, 3123, 1]).cuda()
    plain = _model()(mix).detach()
    assert torch.equal(_model("none")(mix).detach(), plain)         # none: the model without the keyword
    assert torch.equal(_model("none")(mix, lens).detach(), plain)
    assert float((plain.sum(1) - mix).abs().max()) > 1e-3           # an untrained model is not consistent
    for mode in K.MODES:
        with torch.no_grad():
            est = _model(mode)(mix)
            cut = _model(mode)(mix, lens)
        _sums_to(est, mix, mode)
        for m, n in enumerate(lens.tolist()):
            _sums_to(cut[m:m + 1, :, :n], mix[m:m + 1, :n], mode)
            assert torch.equal(cut[m, :, n:], plain[m, :, n:])      # the decoder's output beyond the length
    with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
        est = _model("power")(mix, lens)
    assert est.dtype == torch.float32
    _sums_to(est[:1], mix[:1], "bf16")


def _solver_run(tmp_path, loss, C, mode, seed=0):
    """Two training steps and one validation step of the small model on synthetic.py batches."""
    import conv_tasnet as ct
    import ctn_optim
    import synthetic
    import train
    from solver import Solver
    args = train.parser.parse_args(["--loss", loss, "--C", str(C), "--batch_size", "4", "--epochs", "1",
                                    "--mixture_consistency", mode, "--print_freq", "1",
                                    "--save_folder", str(tmp_path / loss)])
    train.check_mixit(args)
    train.check_mixture_consistency(args)
    batches = []
    for i in range(3):
        mix, src = synthetic.speech_like(4 if i < 2 else 1, 2, 2000, seed + 10 * i)
        lens = torch.tensor([2000, 1800, 2000, 1500][:mix.size(0)])
        for b, n in enumerate(lens):
            mix[b, n:] = 0
            src[b, :, n:] = 0
        batches.append((mix, lens, src))
    torch.manual_seed(seed)
    cfg = CFG[:-1] + (C,)
    model = train.Single(ct.ConvTasNet(*cfg, mixture_consistency=args.mixture_consistency).cuda())
    before = [p.detach().clone() for p in model.parameters()]
    solver = Solver({"tr_loader": batches[:2], "cv_loader": batches[2:]}, model,
                    ctn_optim.Adam(model.parameters(), lr=1e-3), args)
    out = io.StringIO()
    with redirect_stdout(out):
        solver.train()
    return out.getvalue(), before, [p.detach().clone() for p in model.parameters()], solver


@pytest.mark.parametrize("loss,C,mode", [("mixit", 4, "power"), ("pit", 2, "uniform")])
def test_solver_trains_with_mixture_consistency(tmp_path, loss, C, mode):
    text, before, after, solver = _solver_run(tmp_path, loss, C, mode)
    assert text.count("| Iter ") == 3
    assert np.isfinite(float(solver.tr_loss[0])) and np.isfinite(float(solver.cv_loss[0]))
    assert any(not torch.equal(a, b) for a, b in zip(before, after))
    assert all(torch.isfinite(p).all() for p in after)
    pkg = torch.load(os.path.join(tmp_path / loss, "final.pth.tar"), weights_only=True)
    assert pkg["mixture_consistency"] == mode


def test_chunked_separator_keeps_the_sum():
    """Three windows of 4000 with overlap 1000 over T = 9000 (the last window holds 3000
    samples and 1000 zeros): every window sums to its input and the fade weights sum to one,
    so the stitched estimates sum to the mixture within 8 C 2^-24 max(|x[t]|, max_c |y_c[t]|):
    the roundings of the projection, of the cross-fade and of the fade pair."""
    import longform
    import synthetic
    mix, _ = synthetic.speech_like(1, 2, 9000, 12)
    mix = mix[0].cuda()
    chunker = longform.ChunkedSeparator(_model("power"), 4000, 1000, batch=2)
    assert longform.window_count(9000, 4000, 1000) == 3
    y = chunker.separate(mix)
    assert y.shape == (4, 9000)
    bound = 8 * 4 * 2.0 ** -24 * torch.maximum(mix.double().abs(), y.double().abs().amax(0))
    gap = (y.double().sum(0) - mix.double()).abs() - bound
    print(f"chunked: worst |sum - x| / bound {float(((y.double().sum(0) - mix.double()).abs() / bound).max()):.3f}")
    assert float(gap.max()) <= 0.0, float(gap.max())
    plain = longform.ChunkedSeparator(lambda w: _model("none")(w), 4000, 1000, batch=2).separate(mix)
    assert plain.shape == (4, 9000)                                  # any other callable: called as before


def test_power_package_loads_in_evaluate_and_separate(tmp_path):
    """A package written with mixture consistency on carries the mode into evaluate.py and
    separate.py, whose estimates then add up to the mixture within each length."""
    import conv_tasnet as ct
    import evaluate
    import separate
    import synthetic
    model = _model("power", seed=3)
    path = str(tmp_path / "power.pth.tar")
    torch.save(ct.ConvTasNet.serialize(model, torch.optim.SGD(model.parameters(), lr=0.1), 1), path)
    mix, _ = synthetic.speech_like(2, 2, 4000, 13)
    lens = torch.tensor([4000, 2999])
    with redirect_stdout(io.StringIO()):
        sep = separate.Separator(path, 8000)
    assert sep.model.mixture_consistency == "power"
    mixes, ests = sep.estimate(mix, lens)
    for x, e in zip(mixes, ests):
        _sums_to(torch.from_numpy(e)[None], torch.from_numpy(x)[None], "separate")
    ev = object.__new__(evaluate.Evaluator)
    ev.model, ev.chunker = ct.ConvTasNet.load_model(path).cuda().eval(), None
    ev.args = evaluate.parser.parse_args(["--model_path", path, "--data_dir", "-"])
    with torch.no_grad():
        est = ev._forward(mix.cuda(), lens.cuda())
    for m, n in enumerate(lens.tolist()):
        _sums_to(est[m:m + 1, :, :n], mix[m:m + 1, :n].cuda(), "evaluate")
