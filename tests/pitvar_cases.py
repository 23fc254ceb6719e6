"""Inputs and fp64 references shared by test_pitvar_cpu.py and test_gpu_pitvar.py (no tests
here): the planted recipe with silent references, an fp64 torch autograd twin of the score at
a given permutation (with switches for the wrong variants the CPU tests rule out), the host
restatement of the backward's coefficient form, and the list of cases both files walk."""
import itertools

import numpy as np
import torch

EPS = 1e-8
MODES = ("snr", "si_snr")


# ---- the planted recipe ----------------------------------------------------------------------
def canonical(perm, silent):
    """The first permutation in itertools order among those that differ from `perm` only in
    which silent reference a quiet output is paired with: the silent references are handed
    out in ascending order to the outputs that have one, in ascending output order."""
    perm = [int(p) for p in perm]
    quiet = [i for i, p in enumerate(perm) if p in silent]
    for i, j in zip(quiet, sorted(perm[i] for i in quiet)):
        perm[i] = j
    return perm


def planted(C, M, T, seed, silent=None, a=0.8, b=0.3, off=0.05, mix_noise=0.0, mixture="sum"):
    """-> (source [M,C,T], est [M,C,T], mixture [M,T] or None, perm [M,C]).  s ~ N(0,1); the
    references of silent[m] are zero; output i follows reference perm[m][i]: est_i = a s + b noise
    + off for an active one, 0.05 noise for a silent one.  mixture: "none" -> None (the loss sums
    the sources), "sum" -> sum_j s_j + mix_noise * noise, "noise" -> the noise term alone.  perm is
    canonical (the first of the permutations that tie exactly over the silent references)."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(M, C, T, generator=g)
    noise = torch.randn(M, C, T, generator=g)
    extra = torch.randn(M, T, generator=g)
    silent = [()] * M if silent is None else silent
    perm = []
    est = torch.zeros(M, C, T)
    for m in range(M):
        for j in silent[m]:
            s[m, j] = 0.0
        p = canonical(torch.randperm(C, generator=g).tolist(), silent[m])
        perm.append(p)
        for i in range(C):
            est[m, i] = 0.05 * noise[m, i] if p[i] in silent[m] else a * s[m, p[i]] + b * noise[m, i] + off
    if mixture == "none":
        mix = None
    elif mixture == "noise":
        mix = (mix_noise if mix_noise else 1.0) * extra
    else:
        mix = torch.zeros(M, T)
        for j in range(C):
            mix = mix + s[:, j]
        mix = mix + mix_noise * extra
    return s.contiguous(), est.contiguous(), mix, torch.tensor(perm)


# ---- the fp64 twin ---------------------------------------------------------------------------
def _active_score(s, e, mode, tau):
    if mode == "snr":
        S, R = (s * s).sum(), ((s - e) ** 2).sum()
        return 10.0 * torch.log10((S + EPS) / (R + tau * S + EPS))
    sc, ec = s - s.mean(), e - e.mean()
    D, Et, Ee = (sc * ec).sum(), (sc * sc).sum(), (ec * ec).sum()
    Pp = D * D * Et / (Et + EPS) ** 2
    Ne = Ee - 2.0 * D * D / (Et + EPS) + D * D * Et / (Et + EPS) ** 2
    return 10.0 * torch.log10(Pp / (Ne + EPS) + EPS)


def _row(source, mixture, m, n, variant):
    """fp64 references, mixture and activity flags of row m cut to n samples."""
    s = source[m, :, :n].double()
    C = s.size(0)
    if mixture is None or variant == "x_from_sources":
        x = torch.zeros(n, dtype=torch.float64)
        for j in range(C):
            x = x + s[j]
    else:
        x = mixture[m, :n].double()
    if variant == "threshold":                       # wrong: silent below -60 dB of unit power
        act = [bool((s[j] * s[j]).mean() > 1e-6) for j in range(C)]
    elif variant == "active_formula":                # wrong: every reference scored as active
        act = [True] * C
    else:
        act = [bool((s[j] != 0).any()) for j in range(C)]
    return s, x, act


def _pair(s, x, act, e, j, mode, tau, tau0):
    if act[j]:
        return _active_score(s[j], e, mode, tau)
    X = (x * x).sum()
    return 10.0 * torch.log10((X + EPS) / ((e * e).sum() + tau0 * X + EPS))


def twin(source, est, lengths, mixture, perm, mode, snr_max=30.0, inactive_snr_max=20.0, w_loss=1.0, w_max=None,
         variant=None):
    """fp64 autograd at a fixed permutation -> (max_snr [M], loss, grad [M,C,T], pair scores
    [M,C]) of w_loss * loss + sum_m w_max[m] * max_snr[m]."""
    M, C, T = est.shape
    tau, tau0 = 10.0 ** (-snr_max / 10.0), 10.0 ** (-inactive_snr_max / 10.0)
    w_max = [0.0] * M if w_max is None else w_max
    e = est.double().clone().requires_grad_(True)
    ms, pairs = [], []
    for m in range(M):
        n = min(int(lengths[m]), T)
        s, x, act = _row(source, mixture, m, n, variant)
        sc = [_pair(s, x, act, e[m, i, :n], int(perm[m][i]), mode, tau, tau0) for i in range(C)]
        total = sc[0]
        for v in sc[1:]:
            total = total + v
        ms.append(total / C)
        pairs.append(torch.stack(sc).detach())
    ms = torch.stack(ms)
    loss = -ms.mean()
    (w_loss * loss + (torch.as_tensor(w_max, dtype=torch.float64) * ms).sum()).backward()
    return ms.detach(), float(loss.detach()), e.grad.detach(), torch.stack(pairs)


def twin_matrix(source, est, lengths, mixture, mode, snr_max=30.0, inactive_snr_max=20.0, variant=None):
    """The C x C scores of every row (output i against reference j) by the twin's formulas
    -> numpy [M,C,C]."""
    M, C, T = est.shape
    tau, tau0 = 10.0 ** (-snr_max / 10.0), 10.0 ** (-inactive_snr_max / 10.0)
    out = np.zeros((M, C, C))
    for m in range(M):
        n = min(int(lengths[m]), T)
        s, x, act = _row(source, mixture, m, n, variant)
        for i in range(C):
            for j in range(C):
                out[m, i, j] = float(_pair(s, x, act, est[m, i, :n].double(), j, mode, tau, tau0))
    return out


def perm_table(C):
    return np.array(list(itertools.permutations(range(C))))


def search(scores, last=False):
    """scores [C,C] -> (perm, sum / C, sums [C!]): the first (or, wrongly, the last) maximum of
    the sequential sums over itertools.permutations."""
    C = scores.shape[0]
    best, bp, sums = None, None, []
    for p in itertools.permutations(range(C)):
        sv = 0.0
        for i in range(C):
            sv += scores[i, p[i]]
        sums.append(sv)
        if best is None or sv > best or (last and sv == best):
            best, bp = sv, p
    return list(bp), best / C, np.array(sums)


# ---- the backward as the library states it -----------------------------------------------------
def restated_grad(source, est, lengths, mixture, perm, mode, snr_max, inactive_snr_max, w_loss, w_max):
    """(al, be, off) per output worked out in fp64 from explicit sums and rounded to fp32,
    scale = fp32(w_max[m]) - fp32(w_loss) / M in fp32, then scale (al s_j + be e_i + off) in fp64,
    rounded to fp32 once.  -> grad [M,C,T] fp32."""
    M, C, T = est.shape
    tau, tau0 = 10.0 ** (-snr_max / 10.0), 10.0 ** (-inactive_snr_max / 10.0)
    out = np.zeros((M, C, T), dtype=np.float32)
    for m in range(M):
        n = min(int(lengths[m]), T)
        s_t, x_t, act = _row(source, mixture, m, n, None)
        s64, x = s_t.numpy(), x_t.numpy()
        scale = np.float32(w_max[m]) - np.float32(w_loss) / np.float32(M)
        for i in range(C):
            j = int(perm[m][i])
            s, e = s64[j], est[m, i, :n].double().numpy()
            if not act[j]:
                X = np.sum(x * x)
                al, be, off = 0.0, -20.0 / (np.log(10.0) * (np.sum(e * e) + tau0 * X + EPS) * C), 0.0
            elif mode == "snr":
                den = np.sum((s - e) ** 2) + tau * np.sum(s * s) + EPS
                al = 20.0 / (np.log(10.0) * den * C)
                be, off = -al, 0.0
            else:
                sb, eb = np.mean(s), np.mean(e)
                sc, ec = s - sb, e - eb
                D, Et, Ee = np.sum(sc * ec), np.sum(sc * sc), np.sum(ec * ec)
                E = Et + EPS
                Pp = D * D * Et / (E * E)
                Nd = Ee - 2.0 * D * D / E + D * D * Et / (E * E) + EPS
                dsnr = 10.0 / (np.log(10.0) * (Pp / Nd + EPS))
                dPp = 2.0 * D * Et / (E * E)
                dNe = -4.0 * D / E + 2.0 * D * Et / (E * E)
                al = dsnr * (dPp * Nd - Pp * dNe) / (Nd * Nd) / C
                be = 2.0 * dsnr * (-Pp / (Nd * Nd)) / C
                off = -al * sb - be * eb
            al, be, off = (float(np.float32(v)) for v in (al, be, off))
            out[m, i, :n] = (float(scale) * (al * s + be * e + off)).astype(np.float32)
    return torch.from_numpy(out)


def row_ratio(got, ref):
    """max over rows (m, c) of max_t |got - ref| / max_t |ref| (rows with ref == 0 must match exactly)."""
    err = (got.double() - ref.double()).abs().amax(-1)
    top = ref.double().abs().amax(-1)
    assert bool((err[top == 0] == 0).all()), "a row whose reference gradient is zero is not zero"
    return float((err[top > 0] / top[top > 0]).max()) if bool((top > 0).any()) else 0.0


def weights(M):
    """Upstream weights of the scalar under test: loss and a weighted max_snr."""
    return 1.0, [0.3 * ((m % 5) - 2) + 0.1 for m in range(M)]


# ---- the shared cases ------------------------------------------------------------------------
# The statistics' chunk rule is the PIT kernels': ceil(T / 2048) chunks, so T = 2049 is one
# sample past a chunk (two chunks of 1025), and 1500 lies inside its first chunk.
def _lengths(T, M):
    return [max(1, v) for v in ([T, (T + 1) // 2, 1, T - 1, T] * 2)[:M]]


def _case(name, C, M, T, seed, silent, mode="snr", lengths=None, planted_perm=True, **kw):
    return dict(name=name, C=C, M=M, T=T, seed=seed, silent=silent, mode=mode,
                lengths=_lengths(T, M) if lengths is None else lengths, snr_max=kw.pop("snr_max", 30.0),
                inactive_snr_max=kw.pop("inactive_snr_max", 20.0), planted_perm=planted_perm, recipe=kw)


def _one(C):
    return (1 % C,)


def _all_but_one(C):
    return tuple(j for j in range(C) if j != C // 2)


CASES = []
for _C in (2, 3, 4, 5, 8):
    for _mode in MODES:
        # rows: all active / one silent / all but one silent; snr_max and the mixture alternate
        CASES.append(_case(f"planted-{_mode}-C{_C}", _C, 3, 300, 100 + _C, [(), _one(_C), _all_but_one(_C)], _mode,
                           lengths=[300, 263, 226], snr_max=30.0 if _C % 2 == 0 else 10.0,
                           mixture="none" if _C in (2, 5) else "sum", mix_noise=0.0 if _C in (2, 5) else 0.5))
for _T in (1, 255, 256, 257, 2049):
    for _mode in MODES:
        # M = 5 rows of lengths T, T/2, 1, T - 1, T; silent patterns cycle over the rows.  At a
        # length of 1 (and at T = 1) the SI-SNR is -80 dB for every pair: those rows tie
        CASES.append(_case(f"edges-{_mode}-T{_T}", 3, 5, _T, 200 + _T, [(), (0,), (2,), (1, 2), ()], _mode,
                           planted_perm=False, mixture="sum" if _T % 2 else "none", mix_noise=0.5))
CASES += [
    _case("mid-chunk-len", 4, 1, 4097, 301, [(3,)], "snr", lengths=[1500], mixture="sum", mix_noise=0.5),
    _case("one-row-C8", 8, 1, 257, 302, [(2, 5)], "si_snr", mixture="none"),
    _case("all-silent-noise-mix", 3, 3, 300, 303, [(0, 1, 2)] * 3, "snr", lengths=[300, 263, 226], mixture="noise"),
    _case("all-silent-no-mix", 4, 3, 300, 304, [(0, 1, 2, 3)] * 3, "si_snr", lengths=[300, 263, 226],
          mixture="none"),
    _case("threshold-regime", 4, 3, 300, 305, [(), (1,), (0, 2)], "snr", lengths=[300, 263, 226], a=1.0, b=1e-3,
          off=0.0, mixture="sum"),
    _case("M257", 2, 257, 64, 306, [((), (0,), (1,))[m % 3] for m in range(257)], "snr",
          lengths=[64 - (m % 7) for m in range(257)], mixture="sum", mix_noise=0.5),
]


def build(case):
    """-> (source, est, mixture or None, lengths tensor, planted perm)."""
    s, e, x, p = planted(case["C"], case["M"], case["T"], case["seed"], silent=case["silent"], **case["recipe"])
    return s, e, x, torch.tensor(case["lengths"]), p


def special(kind):
    """The activity edge cases that are not plain planted recipes -> (case dict, source, est,
    mixture, lengths, planted perm):
      negzero : row 1's silent reference holds -0.0 everywhere;
      beyond  : row 1's reference 1 is non-zero only beyond the length (silent by the contract);
      tiny    : row 1's reference 1 is 1e-6 N(0,1), row 2's is zero but for one denormal sample
                (both active by the contract: there is no threshold)."""
    case = _case(f"special-{kind}", 3, 3, 300, {"negzero": 401, "beyond": 402, "tiny": 403}[kind],
                 [(), (1,), (1,)], "snr", lengths=[300, 263, 226], planted_perm=kind != "tiny", mixture="sum",
                 mix_noise=0.5)
    s, e, x, lens, p = build(case)
    g = torch.Generator().manual_seed(case["seed"] + 1)
    if kind == "negzero":
        s[1, 1] = -0.0
        assert bool(torch.signbit(s[1, 1]).all())
    elif kind == "beyond":
        s[1, 1, 263:] = torch.randn(300 - 263, generator=g)
        s[2, 1, 226:] = 1.0
    else:
        s[1, 1] = 1e-6 * torch.randn(300, generator=g)
        s[2, 1, 17] = 1e-42
        assert 0.0 < float(s[2, 1, 17]) < 1.2e-38
    return case, s, e, x, lens, p
