"""PIT with silent sources (csrc/ctn_pitvar.hip) against fp64 references on the host.

Every case of pitvar_cases.CASES and its three special activity cases is checked the same way
(``_check``) with ``pit_var_criterion.pit_var_host`` (fp64 numpy, every residual formed sample
by sample, itertools.permutations enumerated) and an fp64 torch autograd twin evaluated at the
device's permutation; the device is never compared with itself:

* perm and active equal the host's exactly.  test_pitvar_cpu.py shows why that is legitimate:
  in every row of every case the best permutation sum leads the next distinct one by at least
  1e-3 dB, and the permutations that share it share it bit for bit (first rank wins);
* max_snr and loss are within 2^-23 |ref| + 1e-7 of the reference (fp64 on the device, rounded
  once: the PIT and MixIT kernels' forward bound), and so is the reference's sum of scores at
  the device's permutation;
* the gradient is exactly zero beyond each length, and per row (m, i)
  max_t |dev - ref| <= GRAD_BOUND * max_t |ref|; estimate_source keeps its bits.

GRAD_BOUND: the backward evaluates scale (al s_j + be e_i + off) in fp64 from fp32 coefficients
and rounds once.  Restated on the host (pitvar_cases.restated_grad) against the fp64 twin, the
worst row ratio over all cases of this file is 2.05e-7 (planted-si_snr-C5; the snr cases stay
below 1.4e-7); the bound is 4x that, 8.2e-7.  The MI355X's measured ratios are in DESIGN.md §29.
"""
import ctypes

import pytest
import torch

import pitvar_cases as K

pytestmark = pytest.mark.gpu

GRAD_BOUND = 8.2e-7


def _fwd_bound(ref):
    return 2.0 ** -23 * abs(ref) + 1e-7


def _device(case, s, e, x, lens):
    import pit_var_criterion as pv
    est = e.cuda().requires_grad_(True)
    before = est.detach().clone()
    loss, max_snr, perm, active = pv.cal_loss_var(s.cuda(), est, lens.cuda(), None if x is None else x.cuda(),
                                                  case["mode"], case["snr_max"], case["inactive_snr_max"])
    w_loss, w_max = K.weights(e.size(0))
    (w_loss * loss + (torch.tensor(w_max, device="cuda") * max_snr[:, 0]).sum()).backward()
    assert torch.equal(est.detach(), before), "estimate_source was modified"
    assert max_snr.shape == (e.size(0), 1) and perm.dtype == torch.int64 and active.dtype == torch.bool
    assert perm.shape == active.shape == e.shape[:2]
    assert not perm.requires_grad and not active.requires_grad
    return loss.detach().cpu(), max_snr.detach().cpu()[:, 0], perm.cpu(), active.cpu(), est.grad.cpu()


_HOST = {}


def _host(case, s, e, x, lens):
    """pit_var_host of a case, computed once and shared by the tests that need it."""
    import pit_var_criterion as pv
    if case["name"] not in _HOST:
        _HOST[case["name"]] = pv.pit_var_host(s, e, lens, x, case["mode"], case["snr_max"], case["inactive_snr_max"])
    return _HOST[case["name"]]


def _check(case, s, e, x, lens, planted=None):
    """The general checks of the module docstring -> the measured gradient row ratio."""
    M, C, T = e.shape
    loss, max_snr, perm, active, g = _device(case, s, e, x, lens)
    h = _host(case, s, e, x, lens)
    assert torch.equal(active, torch.from_numpy(h["active"])), (active, h["active"])
    assert torch.equal(perm, torch.from_numpy(h["perm"])), (perm, h["perm"])
    if planted is not None and case["planted_perm"]:
        assert torch.equal(perm, planted)
    for m in range(M):
        best = h["max_snr"][m]
        print(f"{case['name']} row {m}: max_snr {float(max_snr[m]):.6f} ref {best:.6f}")
        assert abs(float(max_snr[m]) - best) <= _fwd_bound(best), (m, float(max_snr[m]), best)
        at_dev = sum(h["scores"][m, i, int(perm[m, i])] for i in range(C)) / C
        assert abs(at_dev - best) <= _fwd_bound(best), (m, perm[m].tolist(), at_dev, best)
        assert not g[m, :, min(int(lens[m]), T):].any()
    print(f"{case['name']}: loss {float(loss):.6f} ref {h['loss']:.6f}")
    assert abs(float(loss) - h["loss"]) <= _fwd_bound(h["loss"]), (float(loss), h["loss"])
    w_loss, w_max = K.weights(M)
    ms, _, gref, _ = K.twin(s, e, lens, x, perm, case["mode"], case["snr_max"], case["inactive_snr_max"], w_loss,
                            w_max)
    for m in range(M):                               # the twin scores the device's permutation
        assert abs(float(max_snr[m]) - float(ms[m])) <= 2 * _fwd_bound(float(ms[m]))
    ratio = K.row_ratio(g, gref)
    print(f"{case['name']}: gradient row ratio {ratio:.3e} (bound {GRAD_BOUND:.2e})")
    assert ratio <= GRAD_BOUND, ratio
    return ratio


@pytest.mark.parametrize("case", K.CASES, ids=[c["name"] for c in K.CASES])
def test_shared_case(case):
    s, e, x, lens, planted = K.build(case)
    _check(case, s, e, x, lens, planted)


@pytest.mark.parametrize("kind", ["negzero", "beyond", "tiny"])
def test_activity_is_exact_zero_inside_the_length(kind):
    """-0.0 is silent; a reference that is non-zero only beyond the length is silent; 1e-6 N(0,1)
    and a single denormal sample are active: there is no threshold."""
    case, s, e, x, lens, planted = K.special(kind)
    _check(case, s, e, x, lens, planted)
    active = _device(case, s, e, x, lens)[3]
    assert active[:, 1].tolist() == ([True, True, True] if kind == "tiny" else [True, False, False])


def test_deterministic():
    for name in ("planted-snr-C8", "planted-si_snr-C8", "edges-snr-T2049"):
        case = next(c for c in K.CASES if c["name"] == name)
        s, e, x, lens, _ = K.build(case)
        a, b = _device(case, s, e, x, lens), _device(case, s, e, x, lens)
        for u, v in zip(a, b):
            assert torch.equal(u, v)


def test_capturable_into_a_graph():
    """Neither call synchronises: forward and backward are captured into a graph whose replay
    on fresh inputs gives the eager call's bits."""
    import pit_var_criterion as pv
    case = next(c for c in K.CASES if c["name"] == "planted-snr-C4")
    src, est, mix, lens, _ = K.build(case)
    lens = lens.cuda()
    s, x = torch.zeros_like(src).cuda(), torch.zeros_like(mix).cuda()
    e = torch.zeros_like(est).cuda().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up outside the capture
        torch.autograd.grad(pv.cal_loss_var(s, e, lens, x)[0], e)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, max_snr, perm, active = pv.cal_loss_var(s, e, lens, x)
        grad, = torch.autograd.grad(loss, e)
    s.copy_(src)
    x.copy_(mix)
    with torch.no_grad():
        e.copy_(est)
    graph.replay()
    torch.cuda.synchronize()
    e2 = est.cuda().requires_grad_(True)
    want = pv.cal_loss_var(src.cuda(), e2, lens, mix.cuda())
    for got, ref in zip((loss, max_snr, perm, active), want):
        assert torch.equal(got, ref)
    assert torch.equal(grad, torch.autograd.grad(want[0], e2)[0])


def test_error_codes_and_bad_arguments():
    """A short workspace returns CTN_ERR_WORKSPACE (3) and C = 1 or 9 CTN_ERR_UNSUPPORTED (2),
    before anything is launched; the Python surface raises."""
    import ctn_lib as L
    import pit_var_criterion as pv
    lib = L.load()
    s, e, x, _ = K.planted(3, 2, 50, seed=1)
    lens = torch.tensor([50, 50]).cuda()
    sd, ed = s.cuda(), e.cuda()
    out = [torch.zeros(64, device="cuda") for _ in range(5)]
    d = L.PitVarDesc(2, 3, 50, 0, 30.0, 20.0)
    nb = lib.ctn_pitvar_workspace_bytes(ctypes.byref(d))
    ws = L.workspace(nb, sd.device)
    call = lambda desc, n: lib.ctn_pitvar_forward(ctypes.byref(desc), sd.data_ptr(), ed.data_ptr(), None,
                                                  lens.data_ptr(), *(o.data_ptr() for o in out), ws.data_ptr(), n, None)
    assert call(d, nb - 1) == 3 and "workspace" in lib.ctn_last_error().decode()
    for C in (1, 9):
        assert call(L.PitVarDesc(2, C, 50, 0, 30.0, 20.0), nb) == 2 and f"C={C}" in lib.ctn_last_error().decode()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pv.cal_loss_var(sd, ed, lens, None, "sdr")
    with pytest.raises(ValueError):
        pv.cal_loss_var(sd[:, :2].contiguous(), ed, lens)
    with pytest.raises(ValueError):
        pv.cal_loss_var(sd, ed, lens, x.cuda()[:, :49])
    with pytest.raises(L.CtnLibraryError):
        pv.cal_loss_var(sd[:, :1].contiguous(), ed[:, :1].contiguous(), lens)
    with pytest.raises(L.CtnLibraryError):
        pv.cal_loss_var(s, e, lens.cpu())                # host tensors: no fallback
