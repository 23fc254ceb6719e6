"""Inputs and fp64 references shared by test_mixit_cpu.py and test_gpu_mixit.py (no tests
here): the planted-assignment recipe, an fp64 torch autograd twin of the MixIT score at a
given assignment, and the host restatement of the backward's coefficient form."""
import numpy as np
import torch

EPS = 1e-8


def planted(C, M, T, seed, a=0.8, b=0.3, off=0.05, scale=1.0):
    """-> (mixtures [M,2,T], est [M,C,T], mask [M] as assignment integers).  Sources
    s_c ~ N(0,1); output 0 goes to recording 0, output C-1 to recording 1, the others at
    random; x_n is the sum of its sources; est = a s + b noise + off."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(M, C, T, generator=g) * scale
    noise = torch.randn(M, C, T, generator=g) * scale
    bits = torch.randint(0, 2, (M, C), generator=g)
    bits[:, 0], bits[:, C - 1] = 0, 1
    mix = torch.zeros(M, 2, T)
    for m in range(M):
        for c in range(C):
            mix[m, int(bits[m, c])] += s[m, c]
    mask = (bits << torch.arange(C)).sum(1)
    return mix, (a * s + b * noise + off).contiguous(), mask


def remix_fp32(est, assign, lengths):
    """remix[m, n] = fp32 sum of the outputs with bit n in ascending c, zero beyond the length."""
    M, C, T = est.shape
    out = torch.zeros(M, 2, T)
    for m in range(M):
        n = int(lengths[m])
        for c in range(C):
            k = (int(assign[m]) >> c) & 1
            out[m, k, :n] = out[m, k, :n] + est[m, c, :n]
    return out


def _side(x, y, mode, tau):
    if mode == "snr":
        X, R = (x * x).sum(), ((x - y) ** 2).sum()
        return 10.0 * torch.log10((X + EPS) / (R + tau * X + EPS))
    xc, yc = x - x.mean(), y - y.mean()
    D, Et, Ee = (xc * yc).sum(), (xc * xc).sum(), (yc * yc).sum()
    Pp = D * D * Et / (Et + EPS) ** 2
    Ne = Ee - 2.0 * D * D / (Et + EPS) + D * D * Et / (Et + EPS) ** 2
    return 10.0 * torch.log10(Pp / (Ne + EPS) + EPS)


def twin(mix, est, lengths, assign, mode, snr_max, w_loss, w_max):
    """fp64 autograd at a fixed assignment -> (max_snr [M], loss, grad [M,C,T]) of
    w_loss * loss + sum_m w_max[m] * max_snr[m]."""
    M, C, T = est.shape
    tau = 10.0 ** (-snr_max / 10.0)
    e = est.double().clone().requires_grad_(True)
    x = mix.double()
    ms = []
    for m in range(M):
        n = int(lengths[m])
        y = [torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)]
        for c in range(C):
            k = (int(assign[m]) >> c) & 1
            y[k] = y[k] + e[m, c, :n]
        ms.append(0.5 * (_side(x[m, 0, :n], y[0], mode, tau) + _side(x[m, 1, :n], y[1], mode, tau)))
    ms = torch.stack(ms)
    loss = -ms.mean()
    (w_loss * loss + (torch.as_tensor(w_max, dtype=torch.float64) * ms).sum()).backward()
    return ms.detach(), float(loss.detach()), e.grad.detach()


def restated_grad(mix, est, lengths, assign, mode, snr_max, w_loss, w_max):
    """The backward as the library states it: (al, be, off) per recording worked out in fp64
    from explicit sums and rounded to fp32, scale = fp32(w_max[m]) - fp32(w_loss) / M in fp32,
    then scale (al x + be y + off) in fp64 with y the fp64 sum of the member outputs,
    rounded to fp32 once.  -> grad [M,C,T] fp32."""
    M, C, T = est.shape
    tau = 10.0 ** (-snr_max / 10.0)
    out = np.zeros((M, C, T), dtype=np.float32)
    x64, e64 = mix.double().numpy(), est.double().numpy()
    for m in range(M):
        n, p = int(lengths[m]), int(assign[m])
        scale = np.float32(w_max[m]) - np.float32(w_loss) / np.float32(M)
        for k in range(2):
            x = x64[m, k, :n]
            y = np.zeros(n)
            for c in range(C):
                if (p >> c) & 1 == k:
                    y = y + e64[m, c, :n]
            if mode == "snr":
                den = np.sum((x - y) ** 2) + tau * np.sum(x * x) + EPS
                al = 10.0 / (np.log(10.0) * den)
                be, off = -al, 0.0
            else:
                xb, yb = np.mean(x), np.mean(y)
                xc, yc = x - xb, y - yb
                D, Et, Ee = np.sum(xc * yc), np.sum(xc * xc), np.sum(yc * yc)
                E = Et + EPS
                Pp = D * D * Et / (E * E)
                Nd = Ee - 2.0 * D * D / E + D * D * Et / (E * E) + EPS
                dsnr = 10.0 / (np.log(10.0) * (Pp / Nd + EPS))
                dPp = 2.0 * D * Et / (E * E)
                dNe = -4.0 * D / E + 2.0 * D * Et / (E * E)
                al = dsnr * (dPp * Nd - Pp * dNe) / (Nd * Nd) / 2.0
                be = 2.0 * dsnr * (-Pp / (Nd * Nd)) / 2.0
                off = -al * xb - be * yb
            al, be, off = (float(np.float32(v)) for v in (al, be, off))
            g = (float(scale) * (al * x + be * y + off)).astype(np.float32)
            for c in range(C):
                if (p >> c) & 1 == k:
                    out[m, c, :n] = g
    return torch.from_numpy(out)


def row_ratio(got, ref):
    """max over rows (m, c) of max_t |got - ref| / max_t |ref| (rows with ref == 0 must match exactly)."""
    err = (got.double() - ref.double()).abs().amax(-1)
    top = ref.double().abs().amax(-1)
    assert bool((err[top == 0] == 0).all()), "a row whose reference gradient is zero is not zero"
    return float((err[top > 0] / top[top > 0]).max()) if bool((top > 0).any()) else 0.0
