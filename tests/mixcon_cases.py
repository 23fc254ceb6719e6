"""Inputs and fp64 references shared by test_mixcon_cpu.py and test_gpu_mixcon.py (no tests
here): the case grid, an fp64 torch autograd twin of the definition, and the host restatement
of the device's evaluation (fp64 sums folded in the device's chunk order, one rounding)."""
import numpy as np
import torch

EPS = 1e-8
MODES = ("uniform", "power")
GRID_T = (1, 5, 2047, 2048, 2049)      # chunk edge (2048 samples per chunk) and odd, unaligned rows
GRID_C = (2, 3, 8, 16)
CLAMP_T = 131073                       # 64 * 2048 + 1: one sample past the 64-chunk cap


def make(M, C, T, seed, resid=0.3, off=0.02):
    """-> (x [M,T], s [M,C,T], g [M,C,T]) fp32: outputs ~ N(0,1) at a different level each,
    the mixture their sum plus a residual, a random upstream gradient."""
    gen = torch.Generator().manual_seed(seed)
    s = torch.randn(M, C, T, generator=gen) * (0.25 + torch.arange(C).float().reshape(1, C, 1) / C) + off
    x = s.double().sum(1).float() + resid * torch.randn(M, T, generator=gen)
    g = torch.randn(M, C, T, generator=gen)
    return x.contiguous(), s.contiguous(), g.contiguous()


def lengths3(T, C):
    """Three utterances: 0 or 1 sample (by the parity of C), some n < T, and T."""
    return torch.tensor([C % 2, max(T - 1 - T // 3, 0), T])


def grid_cases(T):
    """Every (C, M, mode) of the grid at one T -> (name, x, s, g, lengths or None, mode)."""
    for C in GRID_C:
        for M in (1, 3):
            x, s, g = make(M, C, T, seed=1000 * C + 10 * M + T % 7)
            lens = None if M == 1 else lengths3(T, C)
            for mode in MODES:
                yield f"T={T} C={C} M={M} {mode}", x, s, g, lens, mode


def clamp_cases():
    for C in (2, 16):
        x, s, g = make(1, C, CLAMP_T, seed=7 + C)
        for mode, lens in (("power", torch.tensor([CLAMP_T])), ("uniform", torch.tensor([CLAMP_T - 1]))):
            yield f"T={CLAMP_T} C={C} {mode}", x, s, g, lens, mode


def special_cases():
    """Beyond the grid, at T = 2049 (two chunks, odd rows), C = 4, M = 4 with all four kinds of
    length: outputs that already sum to the mixture (r = 0 exactly: multiples of 1/16), all-zero
    outputs, one output 1e4 times louder than the rest."""
    T, C, M = 2049, 4, 4
    lens = torch.tensor([0, 1, 1500, T])
    gen = torch.Generator().manual_seed(77)
    s = torch.randint(-16, 17, (M, C, T), generator=gen).float() / 16.0
    x, _, g = make(M, C, T, seed=78)
    for mode in MODES:
        yield f"r=0 {mode}", s.sum(1).contiguous(), s.contiguous(), g, lens, mode
        yield f"zero outputs {mode}", x, torch.zeros(M, C, T), g, lens, mode
    x, s2, g = make(M, C, T, seed=79)
    s2[:, 1] *= 1e4
    x = (s2.double().sum(1).float() + 0.3 * torch.randn(M, T, generator=gen)).contiguous()
    for mode in MODES:
        yield f"loud output {mode}", x, s2.contiguous(), g, lens, mode


def all_cases():
    for T in GRID_T:
        yield from grid_cases(T)
    yield from clamp_cases()
    yield from special_cases()


def lens_list(lengths, M, T):
    return [T] * M if lengths is None else [min(max(int(v), 0), T) for v in lengths.tolist()]


def twin(x, s, g, lengths, mode):
    """fp64 torch autograd of the definition on the host, from the fp32 inputs ->
    (out [M,C,T], g_est [M,C,T], g_mixture [M,T]) of L = sum(g * out)."""
    M, C, T = s.shape
    sd = s.double().clone().requires_grad_(True)
    xd = x.double().clone().requires_grad_(True)
    outs = []
    for m, n in enumerate(lens_list(lengths, M, T)):
        sm, xm = sd[m, :, :n], xd[m, :n]
        if mode == "power":
            p = (sm * sm).sum(1)
            w = (p + EPS) / (p.sum() + C * EPS)
        else:
            w = torch.full((C,), 1.0 / C, dtype=torch.float64)
        acc = sm[0]
        for c in range(1, C):                                # ascending j
            acc = acc + sm[c]
        r = xm - acc
        outs.append(torch.cat((sm + w[:, None] * r, sd[m, :, n:]), dim=1))
    out = torch.stack(outs)
    (out * g.double()).sum().backward()
    return out.detach(), sd.grad.detach(), xd.grad.detach()


def chunk_fold(v, T):
    """v [..., n] fp64 terms of one utterance (n <= T samples) -> sums [...] in the device's
    order between chunks: ceil(T / 2048) chunks (at most 64) of ceil(T / chunks) samples,
    folded in chunk order (inside a chunk the device adds per thread and wave; numpy pairwise)."""
    chunks = min(max(-(-T // 2048), 1), 64)
    span = -(-T // chunks)
    acc = np.zeros(v.shape[:-1])
    for ch in range(chunks):
        acc = acc + np.sum(v[..., ch * span:min((ch + 1) * span, v.shape[-1])], axis=-1)
    return acc


def restated(x, s, g, lengths, mode):
    """The device's evaluation on the host -> dict(out, g_est [M,C,T], g_mixture [M,T], fp32;
    w [M,C] fp64): fp64 per sample, statistics folded by chunk_fold, every result rounded to
    fp32 once."""
    M, C, T = s.shape
    x64, s64, g64 = x.double().numpy(), s.double().numpy(), g.double().numpy()
    out, gs = s.numpy().copy(), g.numpy().copy()
    gx = np.zeros((M, T), dtype=np.float32)
    ws = np.full((M, C), 1.0 / C)
    for m, n in enumerate(lens_list(lengths, M, T)):
        sm, gm = s64[m, :, :n], g64[m, :, :n]
        acc = np.zeros(n)
        for c in range(C):
            acc = acc + sm[c]
        r = x64[m, :n] - acc
        w, k = ws[m], np.zeros(C)
        if mode == "power":
            p = chunk_fold(sm * sm, T)
            P = 0.0
            for c in range(C):
                P = P + p[c]
            D = P + C * EPS
            w = ws[m] = (p + EPS) / D
            a = chunk_fold(gm * r, T)
            A = 0.0
            for c in range(C):
                A = A + w[c] * a[c]
            k = 2.0 * (a - A) / D
        G = np.zeros(n)
        for c in range(C):
            G = G + w[c] * gm[c]
        out[m, :, :n] = (sm + w[:, None] * r).astype(np.float32)
        gs[m, :, :n] = (gm - G + sm * k[:, None]).astype(np.float32)
        gx[m, :n] = G.astype(np.float32)
    return dict(out=torch.from_numpy(out), g_est=torch.from_numpy(gs), g_mixture=torch.from_numpy(gx), w=ws)


def row_ratio(got, ref):
    """max over rows of max_t |got - ref| / max_t |ref| (a row whose reference is all zero must
    be all zero)."""
    err = (got.double() - ref.double()).abs().amax(-1)
    top = ref.double().abs().amax(-1)
    assert bool((err[top == 0] == 0).all()), "a row whose reference gradient is zero is not zero"
    return float((err[top > 0] / top[top > 0]).max()) if bool((top > 0).any()) else 0.0
