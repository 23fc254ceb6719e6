"""The streaming kernels alone (ctn_stream.hip: the five per-stage "v5" kernels behind
ctn_stream_encode / _block / _decode and the six column-chunked "v7" kernels behind
ctn_stream_call) against an fp64 restatement of the whole-signal causal forward, element by
element, at chunk, ring and call edges.

The C entries are driven directly through ctn_lib, so ring_frames, pos, the dilations, P,
mask_type and ld_samples are free.  The oracle (tests/stream_cases.py, checked without a GPU by
tests/test_stream_oracle.py) is plain torch in float64 on the CPU and knows nothing of chunks,
rings or calls; this file cuts its tensors at the call boundaries.  Every case runs on both
paths:

    v5   stage by stage: w, x0, every block's output and ring rows, the decoded frames, the
         overlap-added samples and the carried tail, after every call
    v7   out, tail_out and every ring after every call, with CTN_SC_W forced to 8 and to 32

Per element |got - ref| <= 1e-4 + 1e-4 |ref| (layers_cases.FP32["y"]); no whole-tensor norm.

State and guards: every ring starts from a finite sentinel that is distinct per slot; after a
call exactly the slots (pos .. pos+K-1) & (R-1) hold the oracle's norm-1 rows and every other
slot is bit-identical to what it was.  Every output, scratch and state buffer has a guard band
behind it that must stay bit-identical, outputs start from 1e4 (an unwritten element fails its
bound), `samples` has ld_samples = needed + 5 with 1e30 in the extra columns, and tail_in
must come back untouched.  A mid-stream start (pos0 = 2^31 - 5, 2^32 - 5) loads the oracle's
prefix rows into the ring slots (pos0 - j) & (R-1) and the prefix's overlap half into tail_in.

What the shapes pin (ST_NT = 256 threads; 8 frames per workgroup, 4 in the v5 decode; column
chunks of SC_W = 8 | 32 outputs summed over 256 / SC_W input slices; sc_width(): 8 while
M * K <= 128):

    H = 1 7 8 9 31 32 33 40 255 256 257 300, B = 1 8 9 33 40, N = 1 9 33 257
                        one chunk short of / on / past a chunk edge for both widths (blockIdx.z > 0,
                        j < n_out false), a second trip of the j += 256 loops, fewer inputs than
                        input slices, every tail of st_matvec's 16-unroll
    M * K = 128, 129    unforced: bit-identical to the forced width on its side of the switch
    K = 1 7 8 9 16 17 3 4 5, twelve K = 1 calls
                        partial frame groups of both group sizes; every overlap from the carried tail
    P = 1 2 3 5 8, dil = 1 2 3 12 64
                        all older taps in the ring (dil > K), all in this call's frames ((P-1) dil < K:
                        the v7 recompute branch), both in one frame; the first (P-1) dil frames of
                        a stream over a ring whose sentinel is not zero
    R == (P-1) dil + K  (3, 12, K 8, R 32), (3, 4, K 8, R 16), (8, 64, K 64, R 512): the tightest
                        ring, three wraps and more; the first two again with R four times larger
    pos0 = 2^31 - 5, 2^32 - 5
                        calls that cross the boundary: (unsigned)src & mask on a long
    L = 2 4 16 40 64, C = 1 2 3 8, M = 1 2 5, relu / softmax / identity, cLN / BN
                        softmax scores pushed to +120 (an unshifted exp overflows from 88.7)

Measured on MI355X, worst error / bound over all cases (the fp32 torch yardstick: 0.068):

    v5   0.082 (frames, softmax C = 8); rings 0.048, block outputs 0.045, x0 0.011, w 0.004
    v7   0.067 (out, softmax H = 33 B = 9); 4 x R: same bits as the tightest ring
    StreamingSeparator 0.026 (BN, softmax)

Checked by changing the kernels for one run each (not kept): `src >= -1` for `src >= 0` in
stream_block_out fails test_v5_stage_by_stage (54 cases) and no test of test_gpu_streaming.py;
`blockIdx.z == 1` on sc_block_out's ring write fails test_v7_call (60); the overlap-add
without `+ prev` fails every test that compares `out`.
"""
import ctypes
import functools

import pytest
import torch

import stream_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64            # floats behind every buffer
UNWRITTEN = 1e4


class Buf:
    """A device buffer with a guard band behind it."""

    def __init__(self, shape, src=None, fill=UNWRITTEN):
        n = 1
        for s in shape:
            n *= int(s)
        self.n = n
        self.flat = torch.empty(n + GUARD, device=DEV)
        self.flat[n:] = _guard()
        self.t = self.flat[:n].view(*shape)
        if src is None:
            self.t.fill_(fill)
        else:
            self.t.copy_(src.to(torch.float32))

    @property
    def ptr(self):
        return self.flat.data_ptr()

    def intact(self):
        return torch.equal(self.flat[self.n:], _guard())


@functools.lru_cache(maxsize=None)
def _guard():
    return -7.0 - torch.arange(GUARD, dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=2)
def device_model(case):
    """The case's parameters on the device in the layouts the kernels read: 1x1 weights
    transposed to [in][out], norms folded to (a, b) pairs."""
    inp = S.make_inputs(case)

    def dev(t):
        return t.contiguous().to(DEV)

    m = {"U": dev(inp["U"]), "g0": dev(inp["g0"]), "b0": dev(inp["b0"]), "wb_t": dev(inp["wb"].t()),
         "wm_t": dev(inp["wm"].t()), "V": dev(inp["V"]), "blocks": []}
    for b in inp["blocks"]:
        n1a, n1b = S.fold_norm(b["n1"])
        n2a, n2b = S.fold_norm(b["n2"])
        m["blocks"].append([dev(t) for t in (b["w1"].t(), b["a1"], n1a, n1b, b["wd"], b["a2"], n2a, n2b, b["w2"].t())])
    return m


def run(case, path, rmul=1):
    """All calls of the case on one path, every exposed tensor compared after every call ->
    (worst ratio per tensor, every output as CPU tensors for bitwise comparisons)."""
    import ctn_lib as L
    lib, st = L.load(), L.stream_handle(torch.device(DEV))
    M, N, Lf, B, H, C, norm, mask, blocks, calls, pos0 = case
    Sh, P = Lf // 2, blocks[0][0]
    ref, inp, mdl = S.reference(case), S.make_inputs(case), device_model(case)
    pre = S.pre_frames(case)
    Rs = [S.ring_frames(case, i, rmul) for i in range(len(blocks))]
    rings = [Buf((M, R, H), src=S.ring_start(case, ref, i, rmul)) for i, R in enumerate(Rs)]
    before = [r.t.cpu() for r in rings]
    tail = Buf((M, C, Sh), src=ref["tail"][:, :, pre - 1] if pre else torch.zeros(M, C, Sh))
    worst, record = {}, []
    if path == "v7":
        barr = (L.StreamBlockParams * max(1, len(blocks)))()
        for i, ((_, dil), b) in enumerate(zip(blocks, mdl["blocks"])):
            barr[i] = L.StreamBlockParams(dil, Rs[i], *(t.data_ptr() for t in b), rings[i].ptr)
        ms = L.StreamModel(*(mdl[k].data_ptr() for k in ("U", "g0", "b0", "wb_t", "wm_t", "V")),
                           ctypes.cast(barr, ctypes.c_void_p), len(blocks))

    for k0, K, pos in S.spans(case):
        d = L.StreamDesc(M, K, N, Lf, B, H, P, C, L.NORM_CLN if norm == "cLN" else L.NORM_BN, S.MASKS.index(mask))
        need = (K - 1) * Sh + Lf
        ld = need + 5
        smp = Buf((M, ld), fill=S.POISON)
        smp.t[:, :need] = inp["samples"][:, k0 * Sh:k0 * Sh + need].to(DEV)
        tail_in = tail.t.clone()
        tail_out, out = Buf((M, C, Sh)), Buf((M, C, K * Sh))
        bufs, got = [smp, tail, tail_out, out] + rings, {}
        if path == "v5":
            w, x = Buf((M, K, N)), Buf((M, K, B))
            L.check(lib.ctn_stream_encode(ctypes.byref(d), smp.ptr, ld, mdl["U"].data_ptr(), mdl["g0"].data_ptr(),
                                          mdl["b0"].data_ptr(), mdl["wb_t"].data_ptr(), w.ptr, x.ptr, st), "encode")
            got["w"], got["x0"] = w.t, x.t
            bufs += [w, x]
            for i, ((_, dil), b) in enumerate(zip(blocks, mdl["blocks"])):
                y = Buf((M, K, B))
                L.check(lib.ctn_stream_block(ctypes.byref(d), dil, pos, Rs[i], x.ptr, *(t.data_ptr() for t in b),
                                             rings[i].ptr, y.ptr, st), "block")
                got[f"y{i}"] = y.t
                bufs.append(y)
                x = y
            frames = Buf((M, C, K, Lf))
            bufs.append(frames)
            L.check(lib.ctn_stream_decode(ctypes.byref(d), x.ptr, w.ptr, mdl["wm_t"].data_ptr(), mdl["V"].data_ptr(),
                                          tail.ptr, tail_out.ptr, frames.ptr, out.ptr, st), "decode")
            got["frames"] = frames.t
        else:
            nb = lib.ctn_stream_workspace_bytes(ctypes.byref(d))
            assert nb > 0 and nb % 4 == 0
            ws = Buf((nb // 4,))
            bufs.append(ws)
            L.check(lib.ctn_stream_call(ctypes.byref(d), ctypes.byref(ms), pos, smp.ptr, ld, tail.ptr, tail_out.ptr,
                                        out.ptr, ws.ptr, nb, st), "call")
        got["out"], got["tail"] = out.t, tail_out.t
        torch.cuda.synchronize()

        exp = {n: ref[n][:, k0:k0 + K] for n in got if n[0] in "wxy"}
        if "frames" in got:
            exp["frames"] = ref["frames"][:, :, k0:k0 + K]
        exp["out"], exp["tail"] = ref["out"][:, :, k0 * Sh:(k0 + K) * Sh], ref["tail"][:, :, k0 + K - 1]
        got = {n: v.cpu() for n, v in got.items()}
        slots = [(pos + f) & (R - 1) for R in Rs for f in range(K)]
        for i, R in enumerate(Rs):
            now = rings[i].t.cpu()
            sl = slots[i * K:(i + 1) * K]
            got[f"ring{i}"], exp[f"ring{i}"] = now[:, sl], ref[f"ring{i}"][:, k0:k0 + K]
            other = torch.ones(R, dtype=torch.bool)
            other[sl] = False
            assert torch.equal(now[:, other], before[i][:, other]), (S.case_id(case), path, f"ring{i}", pos, "stray write")
            before[i] = now
        r = S.ratios(got, exp)
        assert sorted(r) == sorted(got)
        for n, v in r.items():
            worst[n] = max(worst.get(n, 0.0), v)
        assert max(r.values()) <= 1.0, (S.case_id(case), path, pos, K, r)
        for b in bufs:
            assert b.intact(), (S.case_id(case), path, pos, "guard band", tuple(b.t.shape))
        assert torch.equal(tail.t, tail_in) and bool((smp.t[:, need:] == S.POISON).all())
        record.append(got)
        tail = tail_out
    for i in range(len(blocks)):        # the whole ring against the image the oracle predicts
        img = S.ring_image(case, ref, i, len(calls), rmul)
        worst[f"ringimage{i}"] = S.ratio(before[i], img)
        assert worst[f"ringimage{i}"] <= 1.0, (S.case_id(case), path, i)
    S.show(case, path if rmul == 1 else f"{path}-Rx{rmul}", worst)
    return worst, record


def same_bits(a, b):
    return len(a) == len(b) and all(torch.equal(x[n], y[n]) for x, y in zip(a, b) for n in x)


@pytest.mark.parametrize("case", S.ALL_CASES, ids=S.case_id)
def test_v5_stage_by_stage(case, monkeypatch):
    monkeypatch.delenv("CTN_STREAM_GRAPH", raising=False)
    run(case, "v5")


@pytest.mark.parametrize("width", ("8", "32"))
@pytest.mark.parametrize("case", S.ALL_CASES, ids=S.case_id)
def test_v7_call(case, width, monkeypatch):
    monkeypatch.delenv("CTN_STREAM_GRAPH", raising=False)
    monkeypatch.setenv("CTN_SC_W", width)
    run(case, "v7")


@pytest.mark.parametrize("case,side", list(zip(S.WIDTH_CASES, ("8", "32"))), ids=("MK128", "MK129"))
def test_v7_width_switch(case, side, monkeypatch):
    """Unforced, M * K = 128 takes the 8-wide kernels and 129 the 32-wide ones: bit-identical
    to the forced run of that width.  The other width adds the 1x1 sums in another order
    (32 slices instead of 8), so it differs in some bit of some output."""
    monkeypatch.delenv("CTN_STREAM_GRAPH", raising=False)
    monkeypatch.delenv("CTN_SC_W", raising=False)
    assert case[0] * case[9][0] == (128 if side == "8" else 129)
    _, free = run(case, "v7")
    forced = {}
    for w in ("8", "32"):
        monkeypatch.setenv("CTN_SC_W", w)
        forced[w] = run(case, "v7")[1]
    assert same_bits(free, forced[side])
    assert not same_bits(free, forced["8" if side == "32" else "32"])


@pytest.mark.parametrize("path", ("v5", "v7"))
@pytest.mark.parametrize("case", S.RING_CASES, ids=S.case_id)
def test_ring_four_times_larger(case, path, monkeypatch):
    """The tightest-ring cases again with R x 4: the same outputs to the bit (the ring size
    only moves where a row is kept), and the stray-write check over the larger ring."""
    monkeypatch.delenv("CTN_STREAM_GRAPH", raising=False)
    monkeypatch.setenv("CTN_SC_W", "8")
    (P, dil), = case[8]
    assert S.ring_frames(case, 0) == (P - 1) * dil + max(case[9])
    _, tight = run(case, path)
    _, wide = run(case, path, rmul=4)
    for a, b in zip(tight, wide):
        for n in a:
            assert torch.equal(a[n], b[n]), (path, n)


@pytest.mark.parametrize("path", ("v5", "v7"))
def test_same_state_same_bits(path, monkeypatch):
    monkeypatch.delenv("CTN_STREAM_GRAPH", raising=False)
    monkeypatch.setenv("CTN_SC_W", "32")
    assert same_bits(run(S.DETERMINISM_CASE, path)[1], run(S.DETERMINISM_CASE, path)[1])


@pytest.mark.parametrize("case", [S.BASE, S.DETERMINISM_CASE, S.POS_CASES[1]], ids=S.case_id)
def test_v7_direct_launches_match_graph_replay(case, monkeypatch):
    """CTN_STREAM_GRAPH=0 launches the stages directly with pos as a kernel argument; the
    default replays a captured graph that reads pos from the workspace.  Both against the
    oracle, and bit-identical to each other."""
    monkeypatch.setenv("CTN_SC_W", "8")
    monkeypatch.setenv("CTN_STREAM_GRAPH", "0")
    _, direct = run(case, "v7")
    monkeypatch.delenv("CTN_STREAM_GRAPH")
    _, replay = run(case, "v7")
    assert same_bits(direct, replay)


# ----------------------------------------------------------------------------
# the Python layer (streaming.StreamingSeparator) against the same oracle
# ----------------------------------------------------------------------------
def torch_model(case):
    """A causal ConvTasNet holding the case's parameters (blocks with dilations 1, 2, 4, ...)."""
    import conv_tasnet as ct
    M, N, Lf, B, H, C, norm, mask, blocks, calls, pos0 = case
    assert [d for _, d in blocks] == [2 ** i for i in range(len(blocks))] and pos0 == 0
    inp = S.make_inputs(case)
    m = ct.ConvTasNet(N, Lf, B, H, blocks[0][0], len(blocks), 1, C, norm_type=norm, causal=True,
                      mask_nonlinear=mask).to(DEV).eval()

    def put(p, v):
        p.data.copy_(v.to(DEV).reshape(p.shape))

    def put_norm(mod, n):
        if norm == "cLN":
            put(mod.gamma, n["gamma"]), put(mod.beta, n["beta"])
        else:
            put(mod.weight, n["weight"]), put(mod.bias, n["bias"])
            put(mod.running_mean, n["mean"]), put(mod.running_var, n["var"])

    cln, bott, _, maskc = m.separator.network
    put(m.encoder.conv1d_U.weight, inp["U"]), put(m.decoder.basis_signals.weight, inp["V"])
    put(cln.gamma, inp["g0"]), put(cln.beta, inp["b0"]), put(bott.weight, inp["wb"]), put(maskc.weight, inp["wm"])
    for blk, b in zip(m.separator.blocks(), inp["blocks"]):
        ds = blk.net[3].net
        n1, n2 = blk._norms()
        put(blk.net[0].weight, b["w1"]), put(blk.net[1].weight, b["a1"]), put_norm(n1, b["n1"])
        put(ds[0].weight, b["wd"]), put(ds[2].weight, b["a2"]), put_norm(n2, b["n2"]), put(ds[4].weight, b["w2"])
    return m


WIDE = S.mk(H=40, B=24, N=36, L=16, C=3, calls=(40,))
PY_CASES = [("wide", WIDE, 64, (100, 7)), ("one-frame-calls", S.mk(calls=(30,)), 1, (7, 2, 31)),
            ("exact-ring", S.mk(calls=(60,)), 12, (50, 24, 3)),      # (3 - 1) * 2 + 12 = 16 = R
            ("short-pushes", S.mk(L=16, calls=(12,)), 64, (5,)),
            ("BN-softmax", S.mk(norm="BN", mask="softmax", C=3, blocks=((3, 1),), calls=(40,)), 5, (37, 1, 64))]


@pytest.mark.parametrize("one_call", (True, False), ids=("v7", "v5"))
@pytest.mark.parametrize("name,case,max_frames,pushes", PY_CASES, ids=[p[0] for p in PY_CASES])
def test_streaming_separator_against_the_oracle(name, case, max_frames, pushes, one_call, monkeypatch):
    import streaming
    monkeypatch.delenv("CTN_STREAM_GRAPH", raising=False)
    monkeypatch.delenv("CTN_SC_W", raising=False)
    M, Lf, C = case[0], case[2], case[5]
    ref, mix = S.reference(case)["out"], S.make_inputs(case)["samples"].to(DEV)
    s = streaming.StreamingSeparator(torch_model(case), max_frames=max_frames)
    s.one_call = one_call
    if name == "exact-ring":
        s.push(mix[:, :Lf])                     # allocates the rings
        assert s.rings[1].shape[1] == 16 == (3 - 1) * 2 + max_frames
        s.reset()
    parts, i, k, pending = [], 0, 0, 0
    while i < mix.shape[1]:
        n = pushes[k % len(pushes)]
        got = s.push(mix[:, i:i + n])
        pending += min(n, mix.shape[1] - i)
        assert got.shape[:2] == (M, C)
        if pending < Lf:                            # not one whole frame yet: nothing out, samples carried
            assert got.shape[2] == 0 and s.samples.shape[1] == pending
        parts.append(got)
        i, k = i + n, k + 1
    parts.append(s.flush())
    out = torch.cat(parts, dim=2).cpu()
    assert out.shape == ref.shape
    r = {"out": S.ratio(out, ref)}
    S.show(case, f"StreamingSeparator-{name}-{'v7' if one_call else 'v5'}", r)
    assert r["out"] <= 1.0, r
