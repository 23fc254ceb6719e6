"""The oracle and the cases of tests/test_gpu_layers_alone.py checked on their own, without
a GPU (tests/layers_cases.py holds both):

* the same restatement evaluated in float32 stays inside the fp32 bounds on every case,
  so a bound the HIP path misses is the kernels' doing and not the inputs';
* the fp32 cases are conditioned as claimed: |mean| / std >= 1 in the norms' groups, no
  PReLU input and no relu-mask score within 3e-6 x rms of the kink except the exact zeros;
* the cases can fail: every named wrong variant of the oracle (layers_cases.WRONG) is
  rejected by the comparator, with the same bounds, at the case meant to catch it;
* the bf16 cases' inputs are bf16 numbers, and the poisoned cases differ from the zero-padded
  ones in the padded rows only;
* the library rejects the non-causal depthwise call with odd (P - 1) * dilation before it
  touches the device.
"""
import ctypes

import pytest
import torch

import layers_cases as C


@pytest.mark.parametrize("case", C.FP32_CASES, ids=C.case_id)
def test_oracle_fp32_inside_the_fp32_bounds(case):
    ref, cond = C.reference(case)
    C.check_conditioning(case, cond)
    got, _ = C.oracle(case, C.make_inputs(case), torch.float32)
    r = C.ratios(got, ref)
    C.show(case, "fp32-torch", r)
    assert max(r.values()) <= 1.0, r
    K = case[2]
    for n in ("y", "gx"):
        assert torch.count_nonzero(ref[n][:, K:]) == 0 and torch.count_nonzero(got[n][:, K:]) == 0


@pytest.mark.parametrize("case", C.POISON_CASES, ids=C.case_id)
def test_poison_is_confined_to_the_padded_rows(case):
    K = case[2]
    clean, dirty = C.make_inputs(case), C.make_inputs(case, poison=True)
    for n in clean:
        if n in ("x", "gy"):
            assert torch.equal(clean[n][:, :K], dirty[n][:, :K])
            assert not clean[n][:, K:].any() and bool((dirty[n][:, K:].abs() == C.POISON).all())
        else:
            assert torch.equal(clean[n], dirty[n])
    a, b = C.reference(case)[0], C.reference(case, poison=True)[0]
    for n in a:     # the oracle never sees a padded row
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("name", list(C.WRONG))
def test_wrong_variant_is_rejected(name):
    case, poison, must_break = C.WRONG[name]
    assert case in C.FP32_CASES and (not poison or case in C.POISON_CASES)
    inp = C.make_inputs(case, poison=poison)
    ref, _ = C.reference(case, poison=poison)
    # in float32 as well, where that is the point: exp(100) overflows there and not in float64
    for dtype in (torch.float64, torch.float32):
        got, _ = C.oracle(case, inp, dtype, wrong=name.replace("_cln", "").replace("_causal", ""))
        r = C.ratios(got, ref)
        C.show(case, f"{name}-{str(dtype)[6:]}", r)
        if name == "softmax_no_max" and dtype == torch.float64:
            assert max(r.values()) <= 1.0, r      # only the arithmetic's range tells the two apart
            continue
        for n in must_break:
            assert r[n] > 10.0, (name, n, r)


def test_softmax_no_max_passes_at_80_alone():
    """Why the mask cases also carry +-100: in float32 the variant without the max subtraction
    is still right at +-80."""
    s = torch.tensor([[80.0, -80.0, 80.0], [-80.0, -80.0, -80.0]])
    e = torch.exp(s)
    assert torch.isfinite(e).all() and torch.allclose(e / e.sum(1, keepdim=True), torch.softmax(s.double(), 1).float())
    e = torch.exp(torch.tensor([100.0, -100.0]))
    assert torch.isinf(e[0]) and not torch.isfinite(e / e.sum()).all()


@pytest.mark.parametrize("case", C.BF16_CASES, ids=C.case_id)
def test_bf16_inputs_are_representable(case):
    inp = C.make_inputs(case, bf16=True)
    for n in ("x", "gy"):
        assert torch.equal(inp[n], inp[n].bfloat16().float())
    assert not torch.equal(inp["x"], C.make_inputs(case)["x"])
    # and the bf16 bound is the wider one only for the stored bf16 tensors
    ref, _ = C.reference(case, bf16=True)
    b32, b16 = C.bounds(ref), C.bounds(ref, bf16=True)
    for n in ref:
        assert b16[n] == ((2.0 ** -8, b32[n][1]) if n in ("y", "gx") else b32[n])


def test_case_tables_reach_the_paths_they_name():
    """The constants the cases were chosen against (ctn_layers.hip, ctn_reduce.hip)."""
    nb = [-(-K // C.LY_RB) for _, _, K, _ in C.LN_CASES[:9]]
    assert nb == [1, 1, 1, 2, 2, 3, 7, 8, 9]               # thread < 2 <= tile < 8 <= block
    assert [M * C.padded(K) // C.LY_RB for M, K in C.PARTS_TABLE] == [2, 30, 32, 34, 66]
    M, K, ch = C.BIG
    assert M * C.padded(K) * ch > 4096 * 256                # a second grid-stride trip
    assert C.padded(128) == 128 and C.padded(129) == 256 and C.padded(1) == 128
    assert sorted({c[3] * c[4] % 4 == 0 for c in C.DW_CASES}) == [False, True]   # scalar and vec4 slab_reduce
    for P, dil in C.DW_UNSUPPORTED:
        assert (P - 1) * dil % 2 == 1
    for c in C.DW_CASES:
        assert c[6] or (c[4] - 1) * c[5] % 2 == 0


def test_library_rejects_odd_noncausal_depthwise_without_a_device():
    import ctn_lib as L
    lib = L.load()
    d = L.RowsDesc(2, 128, 128, 8, L.DTYPE_F32)
    for P, dil in C.DW_UNSUPPORTED:
        assert lib.ctn_depthwise_forward(ctypes.byref(d), P, dil, 0, None, None, None, None) == 2
        assert "odd" in lib.ctn_last_error().decode()
        assert lib.ctn_depthwise_backward(ctypes.byref(d), P, dil, 0, None, None, None, None, None, None, 0, None) == 2
        assert "odd" in lib.ctn_last_error().decode()
        # the causal call with the same taps is supported: it gets as far as the pointer check
        assert lib.ctn_depthwise_forward(ctypes.byref(d), P, dil, 1, None, None, None, None) == 1
        assert "null pointer" in lib.ctn_last_error().decode()
