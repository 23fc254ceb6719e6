"""The oracle and the cases of tests/test_gpu_stream_alone.py checked on their own, without a
GPU (tests/stream_cases.py holds both):

* the same restatement evaluated in float32 stays inside the per-element fp32 bound
  (layers_cases.FP32["y"]: 1e-4 + 1e-4 |ref|) against float64 on every case, and uses at most
  half of it, so a bound the HIP path misses is the kernels' doing and not the inputs';
* the inputs are what the generator promises: every compared tensor has rms in [0.1, 10], the
  softmax cases' scores pass +100 (exp overflows float32 from 88.7: +-80 alone would let a
  softmax without the max subtraction through), the mid-stream cases carry a prefix of at
  least max (P-1)*dil frames, and the tables reach the edges they name;
* the cases can fail: every named wrong variant (stream_cases.WRONG) is rejected by the
  comparator at the case meant to catch it, on the tensors it names, and stays inside the
  bound on the tensors upstream of the defect.  For the variants that touch few elements the
  whole-tensor L2 figure of tests/test_gpu_streaming.py (rel() < 1e-5 against the HIP forward,
  < 1e-4 against the golden file) is printed next to it;
* the four C entries of streaming validate their arguments before they touch the device.
"""
import ctypes

import pytest
import torch

import stream_cases as S


@pytest.mark.parametrize("case", S.ALL_CASES + [S.DETERMINISM_CASE], ids=S.case_id)
def test_oracle_fp32_inside_half_the_bound(case):
    ref = S.reference(case)
    got = S.oracle(case, S.make_inputs(case), torch.float32)
    r = S.ratios(got, ref)
    S.show(case, "fp32-torch", r)
    assert sorted(r) == sorted(n for n in ref if n != "score")
    assert max(r.values()) <= 0.5, r


@pytest.mark.parametrize("case", S.ALL_CASES + [S.DETERMINISM_CASE], ids=S.case_id)
def test_inputs_are_what_the_generator_promises(case):
    M, N, L, B, H, C, norm, mask, blocks, calls, pos0 = case
    ref, inp = S.reference(case), S.make_inputs(case)
    for n, v in ref.items():
        if n != "score":
            assert 0.1 <= S._rms(v) <= 10.0, (n, S._rms(v))
    assert len({P for P, _ in blocks}) == 1                     # one P per descriptor
    for b in inp["blocks"]:
        for a in (b["a1"], b["a2"]):
            assert 0.15 <= abs(float(a)) <= 0.35
        for n in (b["n1"], b["n2"]):
            assert sorted(n) == (["beta", "gamma"] if norm == "cLN" else ["bias", "mean", "var", "weight"])
            sh = n["beta"] if norm == "cLN" else n["bias"]
            assert float(sh.abs().min()) >= 0.2
    if mask == "softmax":
        assert float(ref["score"].max()) >= 100.0 and float(ref["score"].abs().max()) >= 80.0
        e = torch.exp(ref["score"].float())
        assert not torch.isfinite(e / e.sum(1, keepdim=True)).all()
    if pos0:
        assert S.pre_frames(case) >= max((P - 1) * d for P, d in blocks) > 0
        assert S.spans(case)[0][2] == pos0
    for i, (P, d) in enumerate(blocks):
        R = S.ring_frames(case, i)
        assert R & (R - 1) == 0 and (P - 1) * d + max(calls) <= R < 2 * ((P - 1) * d + max(calls))
        s = S.ring_sentinel(M, R, H)
        assert torch.isfinite(s).all() and (s != 0).all() and len(set(s[0, :, 0].tolist())) == R


def test_case_tables_reach_the_edges_they_name():
    def col(i, cases):
        return [c[i] for c in cases]
    assert col(4, S.COLUMN_CASES[:12]) == [1, 7, 8, 9, 31, 32, 33, 40, 255, 256, 257, 300]
    assert col(3, S.COLUMN_CASES[12:17]) == [1, 8, 9, 33, 40] and col(1, S.COLUMN_CASES[17:]) == [1, 9, 33, 257]
    assert [c[0] * c[9][0] for c in S.WIDTH_CASES] == [128, 129]
    assert set(S.GROUP_CASES[0][9]) == {1, 7, 8, 9, 16, 17, 3, 4, 5}
    assert {P for c in S.TAP_CASES for P, _ in c[8]} == {1, 2, 3, 5, 8}
    assert {d for c in S.TAP_CASES for _, d in c[8]} == {1, 2, 3, 12, 64}
    for c in S.TAP_CASES:       # past the first (P-1)*dil frames of the stream
        assert sum(c[9]) > max((P - 1) * d for P, d in c[8])
    reach = [(P - 1) * d for c in S.TAP_CASES for P, d in c[8]]
    K = 8
    assert any(d > K for c in S.TAP_CASES for P, d in c[8] if P > 1)          # every older tap in the ring
    assert any(0 < r < K for r in reach) and any(r >= K for r in reach)       # own frames only / both kinds
    for c in S.RING_CASES:      # the tightest ring, wrapped three times and more
        (P, d), = c[8]
        assert S.ring_frames(c, 0) == (P - 1) * d + c[9][0] and sum(c[9]) >= 3 * S.ring_frames(c, 0)
    assert S.ring_frames(S.TAP_CASES[-1], 0) == 7 * 64 + 64 == 512
    for c in S.POS_CASES:       # a call that crosses 2^31 or 2^32
        assert any(pos < b <= pos + K - 1 for _, K, pos in S.spans(c) for b in (2 ** 31, 2 ** 32))
    codec = S.CODEC_CASES
    assert {2, 4, 16, 40, 64} <= set(col(2, codec)) and {1, 2, 3, 8} <= set(col(5, codec))
    assert {1, 2, 5} <= set(col(0, codec)) and set(col(7, codec)) == set(S.MASKS) and set(col(6, codec)) == set(S.NORMS)
    case, _, _ = S.WRONG["ring_slot_mod_need"]
    P, d = case[8][1]
    assert S.ring_frames(case, 1) != (P - 1) * d + max(case[9])
    for name, (case, _, _) in S.WRONG.items():
        assert case in S.ALL_CASES, name


@pytest.mark.parametrize("name", list(S.WRONG))
def test_wrong_variant_is_rejected(name):
    case, must_break, must_hold = S.WRONG[name]
    inp, ref = S.make_inputs(case), S.reference(case)
    if name == "ring_slot_mod_need":
        n = len(case[9])
        good, bad = S.ring_image(case, ref, 1, n), S.ring_image(case, ref, 1, n, wrong=name)
        r = {"ringimage1": S.ratio(bad, good)}
        S.show(case, name, r)
        assert r["ringimage1"] > 10.0
        assert S.ratio(S.oracle(case, inp, wrong=None)["out"], ref["out"]) == 0.0     # the outputs cannot tell
        return
    # in float32 as well, where that is the point: exp(100) overflows there and not in float64
    for dtype in (torch.float64, torch.float32):
        got = S.oracle(case, inp, dtype, wrong=name)
        r = S.ratios(got, ref)
        S.show(case, f"{name}-{str(dtype)[6:]}", r)
        if name in S.FEW_ELEMENTS:
            print("REL  ", name, " ".join(f"{n}={S.rel(got[n], ref[n]):.3g}" for n in must_break))
            if name == "cln_eps_outside_sqrt":      # without the quiet frames 2 and 3 nothing can tell
                loud = [k for k in range(S.total_frames(case)) if k not in (2, 3)]
                r_loud = S.ratio(got["x0"][:, loud], ref["x0"][:, loud])
                print("REL  ", name, f"x0 on the loud frames alone: ratio={r_loud:.3g} "
                      f"rel={S.rel(got['x0'][:, loud], ref['x0'][:, loud]):.3g}")
                assert r_loud <= 0.5
        for n in must_hold:
            assert r[n] <= 0.5, (name, n, r)
        if name == "softmax_no_max" and dtype == torch.float64:
            assert max(r.values()) <= 1.0, r      # only the arithmetic's range tells the two apart
            continue
        for n in must_break:
            assert r[n] > 10.0, (name, n, r)


def test_softmax_no_max_passes_at_80_alone():
    """Why the softmax cases' scores are pushed past +100 and not just to 80."""
    s = torch.tensor([[80.0, -80.0, 80.0], [-80.0, -80.0, -80.0]])
    e = torch.exp(s)
    assert torch.isfinite(e).all() and torch.allclose(e / e.sum(1, keepdim=True), torch.softmax(s.double(), 1).float())


def test_fold_norm_matches_eval_batchnorm():
    case = S.CODEC_CASES[-1]
    n = S.make_inputs(case)["blocks"][0]["n1"]
    a, b = S.fold_norm(n)
    y = torch.randn(2, case[4], 5, generator=torch.Generator().manual_seed(1))
    ref = S._norm(y.double(), n, torch.float64, None)
    assert S.ratio(y * a.view(1, -1, 1) + b.view(1, -1, 1), ref) <= 0.5


# ----------------------------------------------------------------------------
# argument validation of ctn_stream_encode / _block / _decode / _call: every check runs before
# the first HIP call, so dummy non-null pointers do (mdl->blocks is a host array)
# ----------------------------------------------------------------------------
ARG, UNSUPPORTED, WORKSPACE = 1, 2, 3
PTR = 0x1000


def _desc(**kw):
    import ctn_lib as L
    d = dict(M=2, K=8, N=12, L=4, B=10, H=14, P=3, C=2, norm=L.NORM_CLN, mask_type=0)
    d.update(kw)
    return L.StreamDesc(*(d[n] for n in ("M", "K", "N", "L", "B", "H", "P", "C", "norm", "mask_type")))


class _Call:
    """One call of each entry with valid dummy arguments; keyword overrides make it invalid."""

    def __init__(self, lib):
        self.lib = lib

    def encode(self, d, ld=None):
        ld = (d.K - 1) * (d.L // 2) + d.L if ld is None else ld
        return self.lib.ctn_stream_encode(ctypes.byref(d), PTR, ld, *([PTR] * 6), None)

    def block(self, d, dil=2, pos=0, R=16, x_in=PTR, x_out=2 * PTR, ring=PTR):
        return self.lib.ctn_stream_block(ctypes.byref(d), dil, pos, R, x_in, *([PTR] * 9), ring, x_out, None)

    def decode(self, d, tail_in=PTR, tail_out=2 * PTR):
        return self.lib.ctn_stream_decode(ctypes.byref(d), PTR, PTR, PTR, PTR, tail_in, tail_out, PTR, PTR, None)

    def call(self, d, pos=0, ld=None, dil=2, R=16, nblocks=1, blocks=True, tail_in=PTR, tail_out=2 * PTR, short=0,
             block_ptr=PTR):
        import ctn_lib as L
        arr = (L.StreamBlockParams * 1)(L.StreamBlockParams(dil, R, *([PTR] * 8), block_ptr, PTR))
        mdl = L.StreamModel(*([PTR] * 6), ctypes.cast(arr, ctypes.c_void_p) if blocks else None, nblocks)
        ld = (d.K - 1) * (d.L // 2) + d.L if ld is None else ld
        nb = self.lib.ctn_stream_workspace_bytes(ctypes.byref(d)) or 1024      # 0: a descriptor it rejects
        return self.lib.ctn_stream_call(ctypes.byref(d), ctypes.byref(mdl), pos, PTR, ld, tail_in, tail_out, PTR, PTR,
                                        nb - short, None)


@pytest.fixture(scope="module")
def entries():
    import ctn_lib as L
    return _Call(L.load())


BAD_DESC = [("L odd", dict(L=5), UNSUPPORTED), ("L = 66", dict(L=66), UNSUPPORTED), ("P = 0", dict(P=0), ARG),
            ("P = 9", dict(P=9), ARG), ("C = 9", dict(C=9), ARG), ("K = 0", dict(K=0), ARG),
            ("gLN", dict(norm=0), UNSUPPORTED), ("mask_type = 3", dict(mask_type=3), ARG)]


@pytest.mark.parametrize("what,kw,code", BAD_DESC, ids=[b[0] for b in BAD_DESC])
def test_every_entry_rejects_a_bad_descriptor(entries, what, kw, code):
    d = _desc(**kw)
    for fn in (entries.encode, entries.block, entries.decode, entries.call):
        assert fn(d) == code, (what, fn.__name__)
        assert entries.lib.ctn_last_error().decode() != ""
    assert entries.lib.ctn_stream_workspace_bytes(ctypes.byref(d)) == 0


def _rejected(entries, rc, code, word):
    assert rc == code, (rc, entries.lib.ctn_last_error().decode())
    assert word in entries.lib.ctn_last_error().decode(), entries.lib.ctn_last_error().decode()


def test_entries_reject_bad_call_arguments(entries):
    d = _desc()                                     # P = 3, K = 8: dil 2 needs 12 frames, dil 4 exactly 16
    e = entries
    _rejected(e, e.block(d, pos=-1), ARG, "pos")
    _rejected(e, e.call(d, pos=-1), ARG, "pos")
    _rejected(e, e.block(d, dil=0), ARG, "dilation")
    _rejected(e, e.call(d, dil=0), ARG, "dilation")
    for R in (12, 24, 0):                           # not a power of two
        _rejected(e, e.block(d, R=R), ARG, "ring_frames")
        _rejected(e, e.call(d, R=R), ARG, "ring_frames")
    # the ring-size rule: (P-1)*d + K = 16 is the tightest ring; the power of two below is short
    _rejected(e, e.block(d, dil=4, R=8), ARG, "ring_frames")
    _rejected(e, e.call(d, dil=4, R=8), ARG, "ring_frames")
    d9 = _desc(K=9)                                 # (P-1)*d + K - 1 = 16 is a power of two and one short
    _rejected(e, e.block(d9, dil=4, R=16), ARG, "ring_frames")
    _rejected(e, e.call(d9, dil=4, R=16), ARG, "ring_frames")
    _rejected(e, e.block(d, x_in=PTR, x_out=PTR), ARG, "alias")
    _rejected(e, e.decode(d, tail_in=PTR, tail_out=PTR), ARG, "alias")
    _rejected(e, e.call(d, tail_in=PTR, tail_out=PTR), ARG, "alias")
    need = (d.K - 1) * (d.L // 2) + d.L
    _rejected(e, e.encode(d, ld=need - 1), ARG, "ld_samples")
    _rejected(e, e.call(d, ld=need - 1), ARG, "ld_samples")
    _rejected(e, e.call(d, short=1), WORKSPACE, "workspace")
    _rejected(e, e.call(d, nblocks=-1), ARG, "nblocks")
    _rejected(e, e.call(d, blocks=False), ARG, "null")
    _rejected(e, e.call(d, block_ptr=None), ARG, "null")
    _rejected(e, e.block(d, ring=None), ARG, "null")
    assert e.lib.ctn_stream_encode(None, PTR, 100, *([PTR] * 6), None) == ARG
    assert "null" in e.lib.ctn_last_error().decode()
