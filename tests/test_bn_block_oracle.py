"""The fp64 oracle of tests/test_gpu_bn_block.py checked on its own, without a GPU:
the same restatement evaluated in float32 stays inside the fp32 bounds the HIP path is held
to, on every case and mode; every case has a channel of PReLU(h1) with |mean|/std >= 1; and
RefBN's buffer semantics are torch.nn.BatchNorm1d's in every mode."""
import numpy as np
import pytest
import torch

import test_gpu_bn_block as T

ALL = [(c, "train") for c in T.TRAIN_CASES + [T.LARGE_MEAN_CASE]] + [(T.MODE_CASE, m) for m in T.MODES if m != "train"]


@pytest.mark.parametrize("case,mode", ALL, ids=lambda v: v if isinstance(v, str) else T.case_id(v))
def test_oracle_fp32_inside_the_fp32_bounds(case, mode):
    ref, counts, cond = T.reference(case, mode)
    T.check_conditioning(cond)
    got, counts32, _ = T.run_oracle(case, mode, torch.float32)
    assert counts == counts32
    for g, r in zip(got, ref):
        bounds = T.fp32_bounds(r)
        gt, rt = T.tensors(g), T.tensors(r)
        ratios = {n: T.worst(gt[n], rt[n], *bounds[n]) for n in rt}
        print(T.case_id(case), mode, "fp32 torch error / bound:", {n: f"{v:.3g}" for n, v in ratios.items()})
        assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("mode", list(T.MODES))
def test_refbn_is_batchnorm1d(mode):
    momentum, track, training, calls = T.MODES[mode]
    g = torch.Generator().manual_seed(5)
    H = 8
    mean, var = torch.randn(H, generator=g).double(), 0.5 + torch.rand(H, generator=g).double()
    w, b = torch.randn(H, generator=g).double(), torch.randn(H, generator=g).double()
    bn = torch.nn.BatchNorm1d(H, eps=1e-4, momentum=momentum, track_running_stats=track).double().train(training)
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
        if track:
            bn.running_mean.copy_(mean)
            bn.running_var.copy_(var)
    mine = T.RefBN(mean, var, momentum, 1e-4, track, training)
    for _ in range(3):
        x = torch.randn(3, H, 5, generator=g).double() + 1.0
        assert torch.equal(bn(x), mine(x, w, b))
        if track:
            assert torch.equal(bn.running_mean, mine.mean) and torch.equal(bn.running_var, mine.var)
            assert int(bn.num_batches_tracked) == mine.count
        else:
            assert bn.running_mean is None and mine.mean is None and mine.count is None


@pytest.mark.parametrize("case", T.BF16_CASES, ids=T.case_id)
def test_bf16_cases_are_conditioned_and_representable(case):
    ref, counts, cond = T.reference(case, "train")
    T.check_conditioning(cond, fp32=False)
    xs, Gs, params, bufs = T.make_inputs(case)
    for t in (xs[0], params[0], params[8]):
        assert torch.equal(t, t.bfloat16().float())
    got, _, _ = T.run_oracle(case, "train", torch.float32)
    assert T.rel(got[0][0], ref[0][0]) < 1e-5 and T.rel(got[0][1], ref[0][1]) < 1e-3
