"""Golden vectors for the PIT loss with the source left NONZERO beyond each length, captured
from the REAL reference (build container only; the same import shim as make_golden.py, whose
helpers this reuses).

Run from the repo root:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pit_edges.py

pit_edges.npz : cal_loss and cal_si_snr_with_pit (pit_criterion.py:12-113) at C = 1, 2, 4, 7,
                M = 3, T = 600, lengths 600, 431, 257.  Every other PIT fixture zeroes the
                source beyond the lengths, where the reference's source mean over ALL t
                (pit_criterion.py:42) equals the mean over t < length; here the two differ, so
                these vectors pin which of them the mean, the target energy and the dot
                products use.  Keys as in pit_wide.npz, plus .idx (the argmax, :72).
"""
import numpy as np
import torch

import make_golden as mg

M, T, LENS = 3, 600, [600, 431, 257]


def pit_edges_fixtures():
    rng = np.random.default_rng(2049)
    out = {}
    for C in (1, 2, 4, 7):
        # not zeroed beyond LENS; on a 2^-12 grid, which deflates (the file stays under 400 kB)
        src = (np.round(rng.standard_normal((M, C, T)) * 4096) / 4096).astype(np.float32)
        perm = [list(rng.permutation(C)) for _ in range(M)]
        est = np.stack([src[b, perm[b]] for b in range(M)]) * 0.8 + \
            0.5 * rng.standard_normal((M, C, T)).astype(np.float32) + 0.3
        s = torch.from_numpy(src)
        e = torch.from_numpy(est.astype(np.float32)).requires_grad_(True)
        e2 = e * 1.0
        lengths = torch.tensor(LENS)
        loss, max_snr, est_m, reord = mg.ref_pit.cal_loss(s, e2, lengths)
        loss.backward()
        _, _, idx = mg.ref_pit.cal_si_snr_with_pit(s, (e * 1.0).detach(), lengths)
        k = f"pit.C{C}.nz"
        out.update({k + ".src": s, k + ".est": e.detach(), k + ".len": lengths,
                    k + ".loss": loss.detach(), k + ".max_snr": max_snr.detach(),
                    k + ".est_m": est_m.detach(), k + ".reord": reord.detach(),
                    k + ".gest": e.grad, k + ".idx": idx, k + ".perm": np.array(perm)})
    mg.save("pit_edges.npz", **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    pit_edges_fixtures()
