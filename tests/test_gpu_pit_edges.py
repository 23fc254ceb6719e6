"""The PIT loss kernels on their own (ctn_pit.hip: statistics, permutation search, reorder,
backward) against an fp64 reference, at the chunk, length, batch and tie edges that the
fixtures (T <= 1000, M <= 3, source zeroed beyond each length) never reach.

Reference (CPU, float64): the oracle's two-pass pairwise SI-SNR (O.si_snr_pairwise, pinned to
the reference with a source that is NOT zeroed beyond the lengths by pit_edges.npz,
tests/test_oracle_golden.py), the permutation by enumeration in itertools order (C <= 7, first
maximum, with the gap to the runner-up) or by assignment (C >= 8), the gradient by autograd of
the scalar under test, the masked and reordered estimates by plain indexing.

The source stays nonzero beyond each length, so the source sum over all t (the mean,
pit_criterion.py:42) and the one over t < length (target energy, dot products, the backward
offset) differ: mixing the two up anywhere fails here.

Bounds.  max_snr and loss: |dev - ref| <= 2^-23 |ref| + 1e-7 (formed in fp64 on the device,
rounded once to fp32).  Gradient, per row (m, i): max_t |dev - ref| <= 4e-6 max_t |ref| (fp32
coefficients and an fp32 scale (al s + be e + off); a CPU restatement gives 6.7e-7), exactly 0
for t >= length.  Measured on one MI355X: forward at most 0.40 of its bound, gradient 3.4e-7
(8.0e-6 of 3e-5 at a DC offset of 100); per family in DESIGN.md, "PIT edges".  GPU only.
"""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import ctn_oracle as O
from test_gpu_model import DEV, T, load

pytestmark = pytest.mark.gpu

FWD_REL, FWD_ABS = 2.0 ** -23, 1e-7
GRAD_REL = 4e-6


def make_inputs(C, M, Tn, lens, seed, offset=0.3):
    """The fixtures' recipe (make_golden_wide.py), the source left nonzero beyond the lengths."""
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((M, C, Tn)).astype(np.float32)
    perm = np.stack([rng.permutation(C) for _ in range(M)])
    est = (np.stack([src[b, perm[b]] for b in range(M)]) * 0.8
           + 0.5 * rng.standard_normal((M, C, Tn)).astype(np.float32) + offset).astype(np.float32)
    return src, est, torch.tensor(list(lens), dtype=torch.int64), perm


def perm_sums(snr):
    """[M, C!] sums over i of snr[m, i, p[i]], permutations in itertools order (C <= 7)."""
    C = snr.shape[1]
    perms = np.array(list(itertools.permutations(range(C))))
    return snr[:, np.arange(C)[None, :], perms].sum(2), perms


def reference(src, est, lens, planted=None, scalar=None, unique=None):
    """fp64 reference of one case -> dict(perm [M,C], rank [M], max_snr [M], loss, grad [M,C,T]
    (of scalar(loss, max_snr [M,1], est_masked), default the loss), est_m, reord (fp32, plain
    indexing), snr [M,C,C]).  Asserts that the chosen permutation is unique by a margin on the
    rows of `unique` (default all)."""
    M, C, Tn = src.shape
    s = torch.from_numpy(src).double()
    e = torch.from_numpy(est).double().requires_grad_(True)
    snr, e_m = O.si_snr_pairwise(s, e, lens)
    snr_n = snr.detach().numpy()
    rows = range(M) if unique is None else unique
    if C <= 7:
        sums, perms = perm_sums(snr_n)
        idx = sums.argmax(1)                       # first maximum
        perm = perms[idx]
        for b in rows:
            gap = sums[b, idx[b]] - np.delete(sums[b], idx[b]).max() if sums.shape[1] > 1 else np.inf
            assert gap >= 1.0, f"utterance {b}: best and second-best permutation {gap:.3g} dB apart"
    else:
        _, perm_t, _, _ = O.si_snr_pit_assign(s, e.detach(), lens)
        perm = perm_t.numpy()
        for b in rows:
            assert planted is not None and perm[b].tolist() == planted[b].tolist()
            for i in range(C):
                j = perm[b, i]
                others = np.concatenate([np.delete(snr_n[b, i], j), np.delete(snr_n[b, :, j], i)])
                assert snr_n[b, i, j] - others.max() >= 10.0, (b, i)
    rank = [O.perm_rank([int(v) for v in p]) for p in perm]
    pt = torch.from_numpy(np.ascontiguousarray(perm))
    max_snr = torch.stack([snr[b, torch.arange(C), pt[b]].sum() for b in range(M)]) / C
    loss = -max_snr.mean()
    (loss if scalar is None else scalar(loss, max_snr.view(M, 1), e_m)).backward()
    est_m = est.copy()
    for b in range(M):
        est_m[b, :, int(lens[b]):] = 0
    reord = np.stack([est_m[b, perm[b]] for b in range(M)])
    return dict(perm=perm, rank=rank, max_snr=max_snr.detach().numpy(), loss=float(loss.detach()),
                grad=e.grad.numpy(), est_m=est_m, reord=reord, snr=snr_n)


def device(src, est, lens, scalar=None):
    """The same on the device through PITFn -> dict(best, max_snr [M], loss, grad, est_m, reord)."""
    import ctn_ops
    est0 = T(est).requires_grad_(True)
    est_d = est0 * 1.0
    loss, max_snr, est_m, best, reord = ctn_ops.PITFn.apply(T(src), est_d, T(lens))
    assert est_m is est_d                      # masked in place, the same object (pit_criterion.py:24)
    (loss if scalar is None else scalar(loss, max_snr, est_m)).backward()
    return dict(best=best.cpu().tolist(), max_snr=max_snr.detach().cpu().numpy().reshape(-1),
                loss=float(loss), grad=est0.grad.cpu().numpy(), est_m=est_m.detach().cpu().numpy(),
                reord=reord.cpu().numpy())


def fwd_excess(dev, ref):
    """|dev - ref| as a fraction of the bound 2^-23 |ref| + 1e-7 (<= 1 passes)."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(dev - ref) / (FWD_REL * np.abs(ref) + FWD_ABS)))


def grad_ratio(gd, gr, lens):
    """Largest per-row max_t |dev - ref| / max_t |ref| over the rows whose reference is not
    identically zero; those rows, and every t >= length, must be exactly zero."""
    worst = 0.0
    for b in range(gr.shape[0]):
        assert not gd[b, :, int(lens[b]):].any(), f"utterance {b}: gradient beyond the length"
        for i in range(gr.shape[1]):
            top = np.abs(gr[b, i]).max()
            if top == 0.0:
                assert not gd[b, i].any(), f"row ({b}, {i}): reference gradient is exactly zero"
                continue
            worst = max(worst, float(np.abs(gd[b, i].astype(np.float64) - gr[b, i]).max() / top))
    return worst


def check(name, src, est, lens, ref, dev, grad_rel=GRAD_REL):
    fm = fwd_excess(dev["max_snr"], ref["max_snr"])
    fl = fwd_excess(dev["loss"], ref["loss"])
    assert dev["best"] == ref["rank"]
    np.testing.assert_array_equal(dev["est_m"], ref["est_m"])
    np.testing.assert_array_equal(dev["reord"], ref["reord"])
    gr = grad_ratio(dev["grad"], ref["grad"], lens)
    dm = float(np.abs(dev["max_snr"].astype(np.float64) - ref["max_snr"]).max())
    print(f"\nPITEDGE {name}: max_snr |diff| {dm:.3e} dB ({fm:.3f} of bound), loss {fl:.3f} of bound, "
          f"grad row ratio {gr:.3e} (bound {grad_rel:.1e})")
    assert fm <= 1.0 and fl <= 1.0, (fm, fl)
    assert gr <= grad_rel, gr


# name: (C, M, T, lengths, seed); what each reaches is in the comment
CASES = {
    "c1_2chunks": (1, 3, 2049, (2049, 1025, 1024), 1),            # span 1025, one permutation
    "c2_3chunks": (2, 4, 4099, (4099, 2734, 1368, 7), 2),         # span 1367: length on a chunk edge, one
                                                                  # past it, two chunks wholly beyond it
    "c3_4chunks": (3, 3, 6145, (6145, 3074, 1537), 3),            # span 1537, short last chunk
    "c4_table": (4, 3, 2500, (2500, 1251, 1250), 4),              # last table-driven C
    "c5_wide": (5, 2, 2300, (2300, 1150), 5),                     # first pit_final_wide C, 2 chunks
    "c7": (7, 2, 2300, (2300, 1150), 7),                          # never launched before
    "c8_stats": (8, 2, 2100, (2100, 1051), 8),                    # last pit_stats_kernel<C>
    "c9_stats_wide": (9, 3, 4500, (4500, 2251, 300), 9),          # pit_stats_wide, 3 chunks of 1500: a
                                                                  # 256-sample tail of 220, nin partial, nin == 0
    "c10_enum": (10, 2, 2050, (2050, 1026), 10),                  # last enumerated C, 2 chunks
    "c11_assign": (11, 2, 2100, (2100, 257), 11),                 # assignment, 2 chunks
    "c13_assign": (13, 2, 2100, (2100, 257), 13),
    "c14_assign": (14, 2, 2100, (2100, 257), 14),
    "c15_assign": (15, 2, 2100, (2100, 257), 15),
    "c16_assign": (16, 2, 2100, (2100, 257), 16),                 # both staging arrays full, values 256..335
    "c2_m300": (2, 300, 64, tuple(64 - (i % 32) for i in range(300)), 22),   # m += 256 of pit_final
    "c5_m300": (5, 300, 64, tuple(64 - (i % 32) for i in range(300)), 25),   # 300 workgroups, pit_loss loop
    "c2_chunk_cap": (2, 2, 270001, (270001, 135000), 27),         # 64 chunks (span 4219); M T and M C T past
                                                                  # the capped reorder / backward grids
}


@pytest.mark.parametrize("name", list(CASES))
def test_pit_edge_case(name):
    C, M, Tn, lens, seed = CASES[name]
    src, est, lens, planted = make_inputs(C, M, Tn, lens, seed)
    ref = reference(src, est, lens, planted)
    assert ref["perm"].tolist() == planted.tolist()       # the planted permutation is the maximum
    check(name, src, est, lens, ref, device(src, est, lens))


@pytest.mark.parametrize("name", ["c2_3chunks", "c9_stats_wide"])
def test_pit_all_three_gradient_inputs(name):
    """loss, max_snr and the masked estimate all carry a gradient into PITFn.backward."""
    C, M, Tn, lens, seed = CASES[name]
    src, est, lens, planted = make_inputs(C, M, Tn, lens, seed)
    rng = np.random.default_rng(1000 + seed)
    a = float(rng.uniform(0.5, 2.0))
    w = rng.standard_normal((M, 1)).astype(np.float32)
    G = (rng.standard_normal((M, C, Tn)) * 1e-4).astype(np.float32)   # the loss gradient's own size

    def scalar(wt, Gt):
        return lambda loss, max_snr, est_m: a * loss + (wt * max_snr).sum() + (Gt * est_m).sum()

    ref = reference(src, est, lens, planted,
                    scalar=scalar(torch.from_numpy(w).double(), torch.from_numpy(G).double()))
    dev = device(src, est, lens, scalar=scalar(T(w), T(G)))
    check(name + "_3grads", src, est, lens, ref, dev)


@pytest.mark.parametrize("C", [3, 4, 5, 6, 11])
def test_pit_exact_tie_takes_first_permutation(C):
    """Two equal estimate rows: exactly two permutations tie (positions 0 and 1 swapped), and
    the first in itertools order wins, as torch.argmax; the assignment path (C = 11) may take
    either (include/ctn.h)."""
    M, Tn, lens = 2, 500, (500, 333)
    src, est, lens, planted = make_inputs(C, M, Tn, lens, 40 + C)
    est[:, 1] = est[:, 0]
    s64, e64 = torch.from_numpy(src).double(), torch.from_numpy(est).double()
    snr = O.si_snr_pairwise(s64, e64, lens)[0].numpy()
    np.testing.assert_array_equal(snr[:, 0], snr[:, 1])
    ranks, vals = [], []
    for b in range(M):
        if C <= 7:
            sums, perms = perm_sums(snr[b:b + 1])
            top = sums[0].max()
            tied = np.flatnonzero(sums[0] >= top - 1e-9)
            assert len(tied) == 2 and top - np.delete(sums[0], tied).max() >= 1.0
            p, q = perms[tied[0]], perms[tied[1]]
            assert p[0] == q[1] and p[1] == q[0] and p[2:].tolist() == q[2:].tolist()
            assert sums[0, tied[0]] == sums[0, tied[1]]        # bit-equal, not only to 1e-9
            ranks.append([int(tied[0]), int(tied[1])])
        else:
            # estimates 2.. dominate their row and column by 10 dB, so estimates 0 and 1 share
            # the two sources left over, either way round
            for i in range(2, C):
                j = planted[b, i]
                others = np.concatenate([np.delete(snr[b, i], j), np.delete(snr[b, :, j], i)])
                assert snr[b, i, j] - others.max() >= 10.0
            p = O.si_snr_pit_assign(s64[b:b + 1], e64[b:b + 1], lens[b:b + 1])[1][0].tolist()
            q = [p[1], p[0]] + p[2:]
            assert sorted(p[:2]) == sorted(planted[b, :2].tolist()) and p[2:] == planted[b, 2:].tolist()
            top = snr[b, np.arange(C), p].sum()
            assert abs(top - snr[b, np.arange(C), q].sum()) <= 1e-9
            ranks.append(sorted([O.perm_rank(p), O.perm_rank(q)]))
        vals.append(top / C)
    if C == 6:   # the cross-thread tie-break of pit_final_wide: the later rank in the lower thread
        assert any(r[1] % 256 < r[0] % 256 for r in ranks), ranks
    dev = device(src, est, lens)
    print(f"\nPITEDGE tie C={C}: ranks {ranks}, device {dev['best']}")
    if C <= 10:
        assert dev["best"] == [r[0] for r in ranks]
    else:
        assert all(dev["best"][b] in ranks[b] for b in range(M))
    assert fwd_excess(dev["max_snr"], vals) <= 1.0
    assert fwd_excess(dev["loss"], -np.mean(vals)) <= 1.0


@pytest.mark.parametrize("C", [2, 5])
def test_pit_length_one(C):
    """A row of length 1: every zero-mean estimate is exactly zero, every pair scores
    10 log10(EPS), the first permutation wins, and the gradient is exactly zero.  (C = 5 caught
    a D whose terms sb SE and n eb sb were left to cancel: a gradient of ~1e-8 on this row.)"""
    M, Tn, lens = 3, 300, (300, 1, 150)
    src, est, lens, planted = make_inputs(C, M, Tn, lens, 60 + C)
    ref = reference(src, est, lens, planted, unique=[0, 2])
    assert ref["rank"][1] == 0 and not ref["grad"][1].any()
    assert abs(ref["max_snr"][1] - 10 * math.log10(1e-8)) < 1e-9
    dev = device(src, est, lens)
    assert np.isfinite(dev["max_snr"]).all() and np.isfinite(dev["grad"]).all() and math.isfinite(dev["loss"])
    assert dev["best"][1] == 0
    assert fwd_excess(dev["max_snr"][1], 10 * math.log10(1e-8)) <= 1.0
    assert not dev["grad"][1].any()
    check(f"length1_C{C}", src, est, lens, ref, dev)


def test_pit_dc_offset():
    """An offset of 100 on an estimate of amplitude ~1: the one-pass fp64 moments still hold
    the forward bound; the fp32 backward's be e + off cancels to be (e - mean) and keeps
    about 2^-24 offset / rms(e - mean) = 6e-6 relative (a CPU restatement: 6.6e-6), bound 3e-5."""
    C, M, Tn, lens = 2, 3, 3000, (3000, 1501, 700)
    src, est, lens, planted = make_inputs(C, M, Tn, lens, 70, offset=100.0)
    ref = reference(src, est, lens, planted)
    check("dc_offset_100", src, est, lens, ref, device(src, est, lens), grad_rel=3e-5)


@pytest.mark.parametrize("C", [1, 2, 4, 7])
def test_pit_edges_vs_reference(C):
    """The device against the reference itself with the source nonzero beyond the lengths
    (pit_edges.npz, tests/golden/make_golden_pit_edges.py), as test_gpu_model.test_pit_loss."""
    import pit_criterion as pc
    g = load("pit_edges.npz")
    k = f"pit.C{C}.nz"
    est0 = T(g[k + ".est"]).requires_grad_(True)
    est = est0 * 1.0
    loss, max_snr, est_m, reord = pc.cal_loss(T(g[k + ".src"]), est, T(g[k + ".len"]))
    assert est_m is est
    loss.backward()
    np.testing.assert_allclose(float(loss), float(g[k + ".loss"]), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(max_snr.detach().cpu().numpy(), g[k + ".max_snr"], rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(est_m.detach().cpu().numpy(), g[k + ".est_m"])
    np.testing.assert_array_equal(reord.cpu().numpy(), g[k + ".reord"])
    np.testing.assert_allclose(est0.grad.cpu().numpy(), g[k + ".gest"], rtol=1e-3, atol=1e-7)
    _, perms, best = pc.cal_si_snr_with_pit(T(g[k + ".src"]), T(g[k + ".est"]), T(g[k + ".len"]))
    assert best.cpu().tolist() == g[k + ".idx"].tolist()
    assert perms.cpu().tolist() == [list(p) for p in itertools.permutations(range(C))]
