"""Windowed separation on the device (csrc/ctn_stitch.hip, longform.py) against
its numpy restatement: the similarity bit for bit in the kernel's summation order and within
fp64 rounding of math.fsum, the permutations, chain and status exactly, the stitched
output bit for bit, and run-to-run identity; then through ``ChunkedSeparator`` with a real
model and with ``separate.py --chunk_s`` and ``evaluate.py --chunk_s``."""
import math
import os

import numpy as np
import pytest
import torch

import longform as lf

pytestmark = pytest.mark.gpu


def planted(C, W, O, T, seed, J=None):
    """Seeded random windows of C planted sources, a random channel order per window, a
    little independent noise per window (so that the cross-fade mixes different numbers),
    and loud samples at both ends of every overlap.  -> (P [J, C, W], tau [J, C])."""
    rng = np.random.default_rng(seed)
    Hs = W - O
    if J is None:
        J = lf.window_count(T, W, O)
    n = (J - 1) * Hs + W
    src = rng.standard_normal((C, n)).astype(np.float32)
    for j in range(1, J):
        for u in (0, O - 1):
            src[:, j * Hs + u] = (rng.standard_normal(C) * 300.0 + np.arange(1, C + 1) * 40.0).astype(np.float32)
    P = np.empty((J, C, W), dtype=np.float32)
    tau = np.empty((J, C), dtype=np.int64)
    for j in range(J):
        tau[j] = rng.permutation(C)
        P[j, tau[j]] = src[:, j * Hs:j * Hs + W] + 1e-3 * rng.standard_normal((C, W)).astype(np.float32)
    return P, tau


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_fsum(P, O, S):
    J, C, W = P.shape
    Hs = W - O
    for j in range(1, J):
        for a in range(C):
            p = P[j - 1, a, Hs:].astype(np.float64)
            for b in range(C):
                pq = p * P[j, b, :O].astype(np.float64)
                assert abs(S[j, a, b] - math.fsum(pq)) <= 1e-12 * np.abs(pq).sum(), (j, a, b)


def run_and_check(P, T, O, fades=("linear", "hann"), fsum=True):
    Pd = torch.from_numpy(P).cuda()
    host = lf.stitch_host(P, T, O, fades[0])
    res = lf.stitch(Pd, T, O, fades[0])
    S = res.sim.cpu().numpy()
    assert (bits(S) == bits(host.sim)).all(), "similarity differs from corr_host"
    if fsum:
        check_fsum(P, O, S)
    assert (res.perm.cpu().numpy() == host.perm).all()
    assert (res.sigma.cpu().numpy() == host.sigma).all()
    assert (res.status.cpu().numpy() == host.status).all()
    out = res.out.cpu().numpy()
    assert out.shape == (P.shape[1], T)
    assert (bits(out) == bits(host.out)).all(), "stitched output differs from ola_host"
    again = lf.stitch(Pd, T, O, fades[0])
    assert torch.equal(again.out, res.out) and torch.equal(again.sim, res.sim)
    assert torch.equal(again.sigma, res.sigma) and torch.equal(again.perm, res.perm)
    for fade in fades[1:]:
        o2 = lf.stitch(Pd, T, O, fade).out.cpu().numpy()
        assert (bits(o2) == bits(lf.ola_host(P, host.sigma, T, O, fade))).all(), fade
    return host, res


_WO = [(64, 1), (64, 32), (1024, 257), (4100, 2049)]


@pytest.mark.parametrize("W,O", _WO)
@pytest.mark.parametrize("C", [2, 3, 4])
def test_stitch_matches_host(C, W, O):
    Hs = W - O
    for k, T in enumerate((W, W + 1, W + 3 * Hs, W + 3 * Hs + 1)):
        P, tau = planted(C, W, O, T, seed=1000 * C + W + k)
        host, _ = run_and_check(P, T, O)
        # the planted chain is what was found
        want = np.stack([tau[j][np.argsort(tau[0])] for j in range(P.shape[0])])
        assert (host.sigma == want).all()
        assert not host.status.any()


def test_stitch_eight_speakers():
    W, O = 1024, 257
    T = W + 3 * (W - O) + 1
    P, tau = planted(8, W, O, T, seed=8)
    host, _ = run_and_check(P, T, O)
    assert (host.sigma == np.stack([tau[j][np.argsort(tau[0])] for j in range(P.shape[0])])).all()


@pytest.mark.parametrize("C,W,O,J", [(3, 64, 31, 300), (2, 16, 8, 1500), (3, 16, 8, 1500)])
def test_chain_scan_across_waves_and_workgroups(C, W, O, J):
    T = W + (J - 1) * (W - O) - 2
    assert lf.window_count(T, W, O) == J
    P, tau = planted(C, W, O, T, seed=J + C)
    host, res = run_and_check(P, T, O)
    assert (host.sigma == np.stack([tau[j][np.argsort(tau[0])] for j in range(J)])).all()
    # the chain really changes along the recording: late windows differ from a scan that
    # stopped at a wave or workgroup edge
    assert len({tuple(r) for r in host.perm[1:].tolist()}) > 1
    assert (res.sigma.cpu().numpy()[[63, 64, 65, 255, 256, 257, J - 1]] == host.sigma[[63, 64, 65, 255, 256, 257, J - 1]]).all()


def test_frame_matches_host():
    for W, O in _WO + [(16, 8)]:
        Hs = W - O
        for T in (1, W - 1, W, W + 1, W + 3 * Hs, W + 3 * Hs + 1, W + 2 * Hs + 5):
            x = np.random.default_rng(T).standard_normal(T).astype(np.float32)
            win = lf.frame(torch.from_numpy(x).cuda(), W, O).cpu().numpy()
            assert (bits(win) == bits(lf.frame_host(x, W, O))).all(), (W, O, T)


def test_identical_channels_tie_to_first_permutation():
    C, W, O = 3, 64, 32
    T = W + 3 * (W - O)
    P, _ = planted(C, W, O, T, seed=5)
    P[2, 1] = P[2, 0]                       # window 2 holds the same signal twice
    host, res = run_and_check(P, T, O)
    S = host.sim
    assert (bits(S[2][:, 0]) == bits(S[2][:, 1])).all() and (bits(S[3][0]) == bits(S[3][1])).all()
    import itertools
    for j in (2, 3):
        scores = [sum(S[j][a][p[a]] for a in range(C)) for p in itertools.permutations(range(C))]
        first = list(itertools.permutations(range(C)))[int(np.argmax(scores))]
        assert scores.count(max(scores)) >= 2, "no exact tie at this boundary"
        assert tuple(res.perm[j].tolist()) == first


def test_nan_in_one_overlap_leaves_the_others():
    C, W, O = 3, 64, 32
    T = W + 4 * (W - O)
    P, _ = planted(C, W, O, T, seed=6)
    clean = lf.stitch_host(P, T, O)
    Pn = P.copy()
    Pn[2, 1, 5] = np.nan                    # in the overlap of windows 1 | 2 only (5 < O)
    host = lf.stitch_host(Pn, T, O)
    res = lf.stitch(torch.from_numpy(Pn).cuda(), T, O)
    assert res.status.tolist() == host.status.tolist() == [0, 0, 1, 0, 0]
    assert res.perm[2].tolist() == [0, 1, 2]
    perm = res.perm.cpu().numpy()
    assert (perm == host.perm).all() and (perm[[1, 3, 4]] == clean.perm[[1, 3, 4]]).all()
    assert (res.sigma.cpu().numpy() == host.sigma).all()
    S = res.sim.cpu().numpy()
    keep = [0, 1, 3, 4]
    assert (bits(S[keep]) == bits(clean.sim[keep])).all()
    assert np.array_equal(np.isnan(S[2]), np.isnan(host.sim[2])) and np.isnan(S[2]).any()
    assert (bits(S[2][~np.isnan(S[2])]) == bits(host.sim[2][~np.isnan(S[2])])).all()
    out = res.out.cpu().numpy()
    assert np.array_equal(np.isnan(out), np.isnan(host.out)) and np.isnan(out).sum() == 1
    ok = ~np.isnan(out)
    assert (bits(out[ok]) == bits(host.out[ok])).all()


# ----------------------------------------------------------------------------
# with a model
# ----------------------------------------------------------------------------
def tiny_model(C):
    import conv_tasnet as ct
    torch.manual_seed(C)
    return ct.ConvTasNet(16, 4, 8, 16, 3, 2, 1, C).cuda().eval()


@pytest.mark.parametrize("C", [2, 3])
def test_short_recording_is_the_plain_forward(C):
    model = tiny_model(C)
    W, O = 200, 100
    sep = lf.ChunkedSeparator(model, W, O, batch=3)
    for T in (1, 57, W):
        x = torch.randn(T, generator=torch.Generator().manual_seed(T)).cuda()
        with torch.no_grad():
            want = model(torch.nn.functional.pad(x, (0, W - T)).unsqueeze(0))[0, :, :T]
        got = sep.separate(x.unsqueeze(0))
        assert got.shape == (C, T) and torch.equal(got, want)
        assert sep.sigma.tolist() == [list(range(C))] and sep.status.tolist() == [0]


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("fade", ["linear", "hann"])
def test_long_recording_matches_host_stitch_of_the_same_outputs(C, fade):
    model = tiny_model(C)
    W, O, batch = 200, 100, 3
    T = W + 2 * (W - O) + 5
    x = torch.randn(T, generator=torch.Generator().manual_seed(11)).numpy()
    win = torch.from_numpy(lf.frame_host(x, W, O)).cuda()
    assert win.shape[0] == 4
    with torch.no_grad():
        P = torch.cat([model(win[b:b + batch]) for b in range(0, win.shape[0], batch)]).cpu().numpy()
    host = lf.stitch_host(P, T, O, fade)
    sep = lf.ChunkedSeparator(model, W, O, batch=batch, fade=fade)
    got = sep.separate(torch.from_numpy(x).cuda())
    assert got.shape == (C, T)
    assert (bits(got.cpu().numpy()) == bits(host.out)).all()
    assert (sep.perm.cpu().numpy() == host.perm).all() and (sep.sigma.cpu().numpy() == host.sigma).all()
    assert (bits(sep.sim.cpu().numpy()) == bits(host.sim)).all() and sep.status.tolist() == [0] * 4
    # under bf16 autocast the forward runs in bf16 and the stitch still gets fp32 windows
    with torch.autocast("cuda", dtype=torch.bfloat16):
        low = sep.separate(torch.from_numpy(x).cuda())
    assert low.dtype == torch.float32 and low.shape == (C, T) and bool(torch.isfinite(low).all())


def test_callable_with_planted_permutations():
    """Any callable [B, W] -> [B, C, W]: scaled copies of the window in an order that changes
    from window to window come back in window 0's order."""
    W, O, C = 64, 24, 3
    gains = torch.tensor([1.0, -0.5, 0.25]).cuda()
    orders = [[2, 0, 1], [0, 1, 2], [1, 2, 0], [2, 1, 0], [0, 2, 1], [1, 0, 2], [2, 0, 1]]
    seen = []

    def model(win):
        out = []
        for w in win:
            tau = orders[len(seen) % len(orders)]
            seen.append(tau)
            y = torch.empty(C, W, device=w.device)
            y[tau] = gains[:, None] * w[None, :]
            out.append(y)
        return torch.stack(out)

    T = W + 5 * (W - O) - 3
    x = torch.randn(T, generator=torch.Generator().manual_seed(3)).cuda()
    sep = lf.ChunkedSeparator(model, W, O, batch=4)
    got = sep.separate(x)
    J = lf.window_count(T, W, O)
    assert len(seen) == J == 6
    inv0 = np.argsort(orders[0])
    assert sep.sigma.tolist() == [[orders[j][inv0[a]] for a in range(C)] for j in range(J)]
    want = (gains[inv0][:, None] * x[None, :])
    assert torch.allclose(got, want, rtol=0, atol=1e-6 * float(x.abs().max()))


def test_separate_cli_chunked(tmp_path):
    """separate.py --chunk_s on two wavs of unequal length: the file names of the plain run,
    the samples of ChunkedSeparator.separate."""
    import conv_tasnet as ct
    import separate
    import synthetic
    from audio_io import read_wav, write_wav
    sr = 8000
    torch.manual_seed(0)
    model = ct.ConvTasNet(16, 4, 8, 16, 3, 2, 1, 2)
    model_path = str(tmp_path / "m.pth.tar")
    torch.save(ct.ConvTasNet.serialize(model, torch.optim.Adam(model.parameters()), 1), model_path)
    mix_dir = tmp_path / "mix"
    os.makedirs(mix_dir)
    lens = (1700, 2900)
    for i, n in enumerate(lens):
        mix, _ = synthetic.speech_like(1, 2, n, 40 + i)
        write_wav(str(mix_dir / f"u{i}.wav"), mix[0].numpy() * (0.3 / float(mix.abs().max())), sr)
    plain, chunked = str(tmp_path / "plain"), str(tmp_path / "chunked")
    base = ["--model_path", model_path, "--mix_dir", str(mix_dir), "--batch_size", "2"]
    separate.separate(separate.parser.parse_args(base + ["--out_dir", plain]))
    separate.separate(separate.parser.parse_args(base + ["--out_dir", chunked, "--chunk_s", "0.1",
                                                         "--chunk_overlap_s", "0.05"]))
    assert sorted(os.listdir(chunked)) == sorted(os.listdir(plain)) and len(os.listdir(plain)) == 6
    dev_model = ct.ConvTasNet.load_model(model_path).cuda().eval()
    sep = lf.from_seconds(dev_model, 0.1, 0.05, sr)
    assert (sep.window, sep.overlap) == (800, 400)
    for i, n in enumerate(lens):
        x, _ = read_wav(str(mix_dir / f"u{i}.wav"))
        est = sep.separate(torch.from_numpy(np.asarray(x, dtype=np.float32)).cuda()).cpu().numpy()
        for c in range(2):
            ref_path = str(tmp_path / f"ref_{i}_{c}.wav")
            write_wav(ref_path, est[c], sr)
            y, _ = read_wav(os.path.join(chunked, f"u{i}_s{c + 1}.wav"))
            assert len(y) == n and np.array_equal(y, read_wav(ref_path)[0])


def test_evaluate_cli_chunked(tmp_path):
    """evaluate.py --chunk_s: every utterance of a padded minibatch is windowed at its own
    length; the SI-SNRi printed is that of ChunkedSeparator's estimates."""
    import conv_tasnet as ct
    import evaluate
    import preprocess
    import synthetic
    from audio_io import write_wav
    from pit_criterion import cal_loss
    sr, root, lens = 8000, str(tmp_path), (1700, 2900)
    kept = {}
    for i, n in enumerate(lens):
        mix, src = synthetic.speech_like(1, 2, n, 50 + i)
        scale = 0.3 / float(mix.abs().max())
        for name, sig in (("mix", mix[0]), ("s1", src[0, 0]), ("s2", src[0, 1])):
            os.makedirs(os.path.join(root, "wav", "tt", name), exist_ok=True)
            write_wav(os.path.join(root, "wav", "tt", name, f"u{i}.wav"), sig.numpy() * scale, sr)
    for name in ("mix", "s1", "s2"):
        preprocess.preprocess_one_dir(os.path.join(root, "wav", "tt", name), os.path.join(root, "json", "tt"), name, sr)
    torch.manual_seed(0)
    model = ct.ConvTasNet(16, 4, 8, 16, 3, 2, 1, 2)
    path = os.path.join(root, "model.pth.tar")
    torch.save(ct.ConvTasNet.serialize(model, torch.optim.Adam(model.parameters()), 1), path)
    args = ["--model_path", path, "--data_dir", os.path.join(root, "json", "tt"), "--batch_size", "2", "--num_workers", "0"]
    ev = evaluate.Evaluator(evaluate.parser.parse_args(args + ["--chunk_s", "0.1", "--chunk_overlap_s", "0.05"]))
    assert (ev.chunker.window, ev.chunker.overlap) == (800, 400)
    ev.run()
    assert len(ev.records) == 2 and all(np.isfinite(r[0]) for r in ev.records)
    assert evaluate.Evaluator(evaluate.parser.parse_args(args)).chunker is None
    # the same figures from ChunkedSeparator directly
    sep = lf.ChunkedSeparator(ct.ConvTasNet.load_model(path).cuda().eval(), 800, 400)
    for mixture, lengths, source in ev.loader:
        mixture, lengths, source = mixture.cuda(), lengths.cuda(), source.cuda()
        est = torch.zeros_like(source)
        for b, n in enumerate(lengths.tolist()):
            est[b, :, :n] = sep.separate(mixture[b, :n])
        _, _, _, paired = cal_loss(source, est, lengths)
        want = evaluate.cal_SISNRi_batch(source, paired, mixture, lengths).cpu().tolist()
    assert [r[0] for r in ev.records] == want
