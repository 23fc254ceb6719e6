"""C-ABI library checks that need no GPU: it loads, reports its ABI, exports
every symbol include/ctn.h declares, and validates arguments (error codes and
messages) before touching the device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ctn.h")


@pytest.fixture(scope="module")
def lib():
    import ctn_lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.fail(f"{L.LIB_PATH} not built (run make / __graft_entry__.build())")
    return L.load()


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ctn_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_entry_points():
    names = declared_functions()
    for must in ("ctn_tblock_forward", "ctn_tblock_backward", "ctn_encoder_forward", "ctn_encoder_backward",
                 "ctn_decoder_forward", "ctn_decoder_backward", "ctn_pit_forward", "ctn_pit_backward"):
        assert must in names


def test_every_declared_symbol_exported(lib):
    import ctn_lib as L
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert set(declared_functions()) == set(L.EXPORTED_SYMBOLS), "ctypes signature table out of sync with ctn.h"


def test_abi_and_padding(lib):
    import ctn_lib as L
    assert lib.ctn_abi_version() == L.ABI_VERSION
    assert lib.ctn_padded_frames(3199) == 3200
    assert lib.ctn_padded_frames(128) == 128
    assert lib.ctn_padded_frames(7999) == 8064


def _desc(**kw):
    import ctn_lib as L
    d = dict(M=2, K=3199, Kp=3200, B=256, H=512, P=3, dilation=4, causal=0, norm_type=0, dtype=1)
    d.update(kw)
    return L.TBlockDesc(**d)


def test_tblock_validation(lib):
    import ctn_lib as L
    ok = _desc()
    assert lib.ctn_tblock_workspace_bytes(ctypes.byref(ok), 0) > 0
    assert lib.ctn_tblock_workspace_bytes(ctypes.byref(ok), 1) > lib.ctn_tblock_workspace_bytes(ctypes.byref(ok), 0)
    assert lib.ctn_tblock_stats_floats(ctypes.byref(ok)) == 4 * 2
    assert lib.ctn_tblock_stats_floats(ctypes.byref(_desc(norm_type=1))) == 4 * 2 * 3200
    bn = _desc(norm_type=2)                         # BatchNorm: per-channel statistics
    assert lib.ctn_tblock_stats_floats(ctypes.byref(bn)) == 4 * bn.H
    assert lib.ctn_tblock_workspace_bytes(ctypes.byref(bn), 1) > 0
    assert lib.ctn_tblock_workspace_bytes(ctypes.byref(_desc(norm_type=3)), 0) == 0
    cases = [(_desc(Kp=3199), L.CtnLibraryError, "multiple of 128"),
             (_desc(P=2), None, "odd P"),
             (_desc(B=100), None, "multiples of 8")]
    for d, _, msg in cases:
        assert lib.ctn_tblock_workspace_bytes(ctypes.byref(d), 0) == 0
        rc = lib.ctn_tblock_forward(ctypes.byref(d), None, None, None, None, None, 0, None)
        assert rc in (1, 2)
        assert msg in lib.ctn_last_error().decode()


def test_forward_rejects_null_and_small_workspace(lib):
    import ctn_lib as L
    d = _desc()
    p = L.TBlockParams()
    sv = L.TBlockSaved()
    assert lib.ctn_tblock_forward(ctypes.byref(d), ctypes.byref(p), None, None, ctypes.byref(sv), None, 0, None) == 1
    assert lib.ctn_pit_forward(None, None, None, None, None, None, None, None, None, None, 0, None) == 1
    pd = L.PitDesc(2, 17, 100)
    assert lib.ctn_pit_workspace_bytes(ctypes.byref(pd)) == 0          # C > 16 unsupported
    pd = L.PitDesc(2, 8, 100)
    assert lib.ctn_pit_workspace_bytes(ctypes.byref(pd)) > 0           # C! = 40,320 permutations


def test_codec_validation(lib):
    import ctn_lib as L
    good = L.CodecDesc(M=2, T=32000, K=3199, Kp=3200, N=256, L=20, B=256, C=2, mask_type=0, dtype=1)
    assert lib.ctn_encoder_workspace_bytes(ctypes.byref(good), 1) > 0
    assert lib.ctn_decoder_workspace_bytes(ctypes.byref(good), 1) > 0
    bad = L.CodecDesc(M=2, T=32000, K=3000, Kp=3072, N=256, L=20, B=256, C=2, mask_type=0, dtype=1)
    assert lib.ctn_encoder_workspace_bytes(ctypes.byref(bad), 0) == 0
    rc = lib.ctn_encoder_forward(ctypes.byref(bad), *([None] * 8), None, 0, None)
    assert rc == 1 and "K=3000" in lib.ctn_last_error().decode()


def test_timer_off_by_default(lib):
    tot, n = ctypes.c_double(1.0), ctypes.c_int(7)
    assert lib.ctn_timer_read(ctypes.byref(tot), ctypes.byref(n)) == 0
    assert n.value == 0 and tot.value == 0.0


def test_timer_stride_validation(lib):
    assert lib.ctn_timer_set_stride(0) != 0
    assert "stride" in lib.ctn_last_error().decode()
    assert lib.ctn_timer_set_stride(8) == 0
    assert lib.ctn_timer_set_stride(1) == 0


def test_copy_validation(lib):
    """ctn_copy_bytes (bench calibration copy) checks sizes and alignment before launching."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.ctn_copy_bytes(None, None, 16, 1, 0, None) == 1
    assert lib.ctn_copy_bytes(p, p, 20, 1, 0, None) == 1       # not a multiple of 16
    assert "16-byte" in lib.ctn_last_error().decode()
    assert lib.ctn_copy_bytes(p, p, 16, 0, 0, None) == 1       # no workgroups
    assert lib.ctn_copy_bytes(p, p, 16, 1, 4, None) == 1       # unknown flag


def test_pack_weights_validation(lib):
    """ctn_pack_weights checks its table before launching anything: an entry needs a
    destination, and the fragment-order copies need rows and cols in multiples of 32."""
    import ctn_lib as L
    assert lib.ctn_pack_weights(None, 0, None) == 0
    empty = (L.WeightPack * 1)(L.WeightPack(16, 64, 64, None, None, None, None))
    assert lib.ctn_pack_weights(empty, 1, None) == 1
    assert "no destination" in lib.ctn_last_error().decode()
    ragged = (L.WeightPack * 1)(L.WeightPack(16, 40, 64, None, None, 256, None))
    assert lib.ctn_pack_weights(ragged, 1, None) == 1
    assert "multiples of 32" in lib.ctn_last_error().decode()
    ragged_t = (L.WeightPack * 1)(L.WeightPack(16, 64, 72, None, None, None, 256))
    assert lib.ctn_pack_weights(ragged_t, 1, None) == 1


def test_device_code_has_no_packed_fp32(tmp_path):
    """The library's gfx950 code objects contain no packed-FP32 VALU instructions
    (v_pk_fma/mul/add_f32): on gfx950 a packed instruction that takes a source half through
    op_sel/op_sel_hi right after the VALU that wrote that register occasionally reads the
    stale value when another wave on the SIMD is busy, and the compiler inserts no wait
    state for it (tools/microbench/pk_hazard.hip).  The Makefile builds with
    the packed-fp32-ops target feature off; this guards against a build without it."""
    import re
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    lib = os.path.join(ROOT, "conv-tasnet_amd", "libctn_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libctn_hip.so not built")
    shutil.copy(lib, tmp_path / "lib.so")
    subprocess.run([objdump, "--offloading", "lib.so"], cwd=tmp_path, check=True, capture_output=True)
    objs = [p for p in os.listdir(tmp_path) if "gfx950" in p]
    assert objs, "no gfx950 code object in the library"
    pk = re.compile(r"\bv_pk_(fma|mul|add)_f32\b")
    n_pk = n_mfma = 0
    for o in objs:
        txt = subprocess.run([objdump, "-d", o], cwd=tmp_path, check=True, capture_output=True, text=True).stdout
        n_pk += len(pk.findall(txt))
        n_mfma += txt.count("v_mfma_")
    assert n_mfma > 0, "disassembly found no MFMA: the check itself is broken"
    assert n_pk == 0, f"{n_pk} packed-FP32 instructions in the device code"


def _plan(lib, backward, **kw):
    buf = ctypes.create_string_buffer(256)
    assert lib.ctn_tblock_plan(ctypes.byref(_desc(**kw)), backward, buf, 256) == 0
    return dict(kv.split("=") for kv in buf.value.decode().split(","))


def test_tblock_plan_bench_shape_and_2gb_fallback(lib):
    """The persistent kernels (weight-stationary GEMMs, wave-specialised dual GEMM,
    wave-item depthwise kernels) address their tiles with 32-bit offsets: at 2^21 frame
    rows (M*Kp*512*2 bytes = 2 GiB) the launch must fall back to the tiled kernels
    (ADVICE r04), while the bench shape takes the persistent ones."""
    fwd, bwd = _plan(lib, 0, M=32), _plan(lib, 1, M=32)
    assert fwd == {"gemm1": "ws", "dw_fwd": "wave", "gemm2": "ws"}, fwd
    assert bwd["pairA"] == "dual_ws" and bwd["dw_bwd"] == "wave" and bwd["gx"] == "ws_n1bwd", bwd
    big = dict(M=656, K=3199, Kp=3200)        # 656 * 3200 = 2,099,200 rows >= 2^21
    fwd, bwd = _plan(lib, 0, **big), _plan(lib, 1, **big)
    assert fwd == {"gemm1": "rows", "dw_fwd": "lane", "gemm2": "rows"}, fwd
    assert bwd["pairA"] not in ("dual_ws", "dual", "ws+cols") and bwd["dw_bwd"] == "lane", bwd
    assert "gx" not in bwd or bwd["gx"] != "ws_n1bwd", bwd
    just_below = dict(M=655, K=3199, Kp=3200)  # 2,096,000 rows
    assert _plan(lib, 1, **just_below)["pairA"] == "dual_ws"


# (M, K, B, H, P, dilation)
_TB_SHAPES = ((2, 3199, 256, 512, 3, 4), (32, 3199, 256, 512, 3, 128), (1, 100, 64, 128, 3, 1),
              (3, 257, 128, 256, 5, 2), (656, 3199, 256, 512, 3, 1),
              # B = 256 with H != 512: pair A stays on the row + column kernels (the dual GEMM
              # takes the 256 -> 512 pair only)
              (32, 3199, 256, 256, 3, 4), (32, 3199, 256, 128, 3, 4))
_F_TILED, _F_FAST = "gemm1=rows,dw_fwd=lane,gemm2=rows", "gemm1=ws,dw_fwd=wave,gemm2=ws"
_B_TILED = "pairA=rows+cols,dw_bwd=lane,n1bwd=ew,gx+dW1=rows+cols"
_B_FAST = "pairA=dual_ws,dw_bwd=wave,gx=ws_n1bwd,dW1=cols"
# (norm, dtype, shape index) -> (workspace fwd, workspace bwd, partials, deferred workspace, plan fwd, plan bwd);
# the recorded values were the same for causal 0 and 1
_TB_RECORDED = {
    (0, 0, 0): (8256, 54950664, 27678984, 27271696, _F_TILED, _B_TILED),
    (0, 0, 1): (119040, 469082228, 48483956, 420598528, _F_TILED, _B_TILED),
    (0, 0, 2): (528, 267520, 69888, 197640, _F_TILED, _B_TILED),
    (0, 0, 3): (1168, 4017408, 1394432, 2623000, _F_TILED, _B_TILED),
    (0, 0, 4): (2120448, 8644686384, 43194160, 8601492352, _F_TILED, _B_TILED),
    (0, 1, 0): (628544, 61793544, 48126984, 13666576, _F_FAST, _B_FAST),
    (0, 1, 1): (672000, 275550324, 65261172, 210289408, _F_FAST, _B_FAST),
    (0, 1, 2): (33296, 169216, 69888, 99336, _F_TILED, _B_TILED),
    (0, 1, 3): (132240, 2706688, 1394432, 1312280, _F_TILED, _B_TILED),
    (0, 1, 4): (2644736, 4345000496, 43194160, 4301806464, _F_TILED, _B_TILED),
    (1, 0, 0): (512256, 55556360, 27678984, 27877632, _F_TILED, _B_TILED),
    (1, 0, 1): (8192256, 478793332, 48483956, 430309632, _F_TILED, _B_TILED),
    (1, 0, 2): (4352, 272640, 69888, 203008, _F_TILED, _B_TILED),
    (1, 0, 3): (55552, 4089600, 1394432, 2695424, _F_TILED, _B_TILED),
    (1, 0, 4): (167936256, 8844089136, 43194160, 8800895232, _F_TILED, _B_TILED),
    (1, 1, 0): (2265344, 62372872, 48126984, 14246144, _F_FAST, _B_FAST),
    (1, 1, 1): (28377344, 285331060, 65261172, 220070144, _F_FAST, _B_FAST),
    (1, 1, 2): (37120, 174336, 69888, 104704, _F_TILED, _B_TILED),
    (1, 1, 3): (186624, 2778880, 1394432, 1384704, _F_TILED, _B_TILED),
    (1, 1, 4): (168460544, 4544403248, 43194160, 4501209344, _F_TILED, _B_TILED),
    (2, 0, 0): (215360, 55157256, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 0, 1): (3302144, 472205916, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 0, 2): (4880, 273408, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 0, 3): (25488, 4045312, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 0, 4): (67214592, 8709699632, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 1, 0): (739648, 41525768, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 1, 1): (3826432, 261966428, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 1, 2): (37648, 175104, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 1, 3): (156560, 2734592, 0, 0, "bn:rows", "bn:rows+cols"),
    (2, 1, 4): (67738880, 4410013744, 0, 0, "bn:rows", "bn:rows+cols"),
    # recorded from the library of commit 8bcfc6c (the last with the tiled dual kernel)
    (0, 0, 5): (64256, 247593044, 37293652, 210299648, _F_TILED, _B_TILED),
    (0, 1, 5): (340736, 142487636, 37293652, 105194240, "gemm1=ws,dw_fwd=lane,gemm2=ws",
                "pairA=ws+cols,dw_bwd=lane,gx=ws_n1bwd,dW1=cols"),
    (1, 0, 5): (4915456, 254086740, 37293652, 216793344, _F_TILED, _B_TILED),
    (1, 1, 5): (15008000, 158797396, 37293652, 121504000, "gemm1=ws,dw_fwd=lane,gemm2=ws",
                "pairA=ws+cols,dw_bwd=lane,gx=ws_n1bwd,dW1=cols"),
    (0, 0, 6): (32512, 140757584, 35605072, 105152768, _F_TILED, _B_TILED),
    (0, 1, 6): (163584, 88197712, 35605072, 52592896, _F_TILED, _B_TILED),
    (1, 0, 6): (3277056, 145640016, 35605072, 110035200, _F_TILED, _B_TILED),
    (1, 1, 6): (3408128, 93080144, 35605072, 57475328, _F_TILED, _B_TILED),
}
# the bf16 gLN bench shape (shape index 1) under one A/B switch each
_TB_RECORDED_ENV = {
    ("CTN_GEMM_DUAL", "0"): (672000, 258805876, 48483956, 210322176, _F_FAST,
                             "pairA=ws+cols,dw_bwd=wave,gx=ws_n1bwd,dW1=cols"),
    # only bit 0 of CTN_GEMM_DUAL is read (pair B's dual kernel is retired)
    ("CTN_GEMM_DUAL", "2"): (672000, 258805876, 48483956, 210322176, _F_FAST,
                             "pairA=ws+cols,dw_bwd=wave,gx=ws_n1bwd,dW1=cols"),
    ("CTN_GEMM_DUAL", "3"): (672000, 275550324, 65261172, 210289408, _F_FAST, _B_FAST),
    ("CTN_FUSE_N1", "0"): (672000, 275550324, 65261172, 210289408, _F_FAST,
                           "pairA=dual_ws,dw_bwd=wave,n1bwd=ew,gx+dW1=rows+cols"),
    # no longer read (the tiled dual kernel it selected is retired): the default plan
    ("CTN_DUAL_WS", "0"): (672000, 275550324, 65261172, 210289408, _F_FAST, _B_FAST),
    ("CTN_DW_WAVE", "0"): (672000, 275550324, 65261172, 210289408, "gemm1=ws,dw_fwd=lane,gemm2=ws",
                           "pairA=dual_ws,dw_bwd=lane,gx=ws_n1bwd,dW1=cols"),
    # no longer read (the dual kernel's column-only mode, the 128-row tiled row GEMM and the
    # column GEMM's workgroup-target override are retired): the default plan.
    # (Before, CTN_COLS_WS=1 and CTN_COLS_WG=512 each gave 292327540 / 82038388 here;
    # CTN_GEMM_BM=128 moved only the shapes that run the tiled row GEMM, not this one.)
    ("CTN_COLS_WS", "1"): (672000, 275550324, 65261172, 210289408, _F_FAST, _B_FAST),
    ("CTN_GEMM_BM", "128"): (672000, 275550324, 65261172, 210289408, _F_FAST, _B_FAST),
    ("CTN_COLS_WG", "512"): (672000, 275550324, 65261172, 210289408, _F_FAST, _B_FAST),
}


def _tb_sizes_and_plans(lib, norm, causal, dtype, shape):
    M, K, B, H, P, dil = shape
    r = ctypes.byref(_desc(M=M, K=K, Kp=lib.ctn_padded_frames(K), B=B, H=H, P=P, dilation=dil, causal=causal,
                           norm_type=norm, dtype=dtype))
    plans = []
    for backward in (0, 1):
        buf = ctypes.create_string_buffer(256)
        assert lib.ctn_tblock_plan(r, backward, buf, 256) == 0
        plans.append(buf.value.decode())
    return (lib.ctn_tblock_workspace_bytes(r, 0), lib.ctn_tblock_workspace_bytes(r, 1),
            lib.ctn_tblock_partials_bytes(r), lib.ctn_tblock_deferred_workspace_bytes(r), plans[0], plans[1])


def test_tblock_sizes_and_plans_match_recorded(lib, monkeypatch):
    """The TemporalBlock's workspace, partials and deferred-workspace byte counts and its
    ctn_tblock_plan strings, for every norm, causality, dtype and a table of shapes, and for
    the bf16 gLN bench shape under each A/B switch.  The expected values were recorded from
    the library of the parent commit of the one that introduced the block plan (TbPlan,
    ctn_capi_tblock.hip), on a machine without a device, where the depthwise segment sizing
    assumes the MI355X's 256 CUs: a refactor of the host driver must leave every one of them
    as it was."""
    for var, _ in _TB_RECORDED_ENV:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.delenv("CTN_WS_FOLD", raising=False)
    for (norm, dtype, i), want in _TB_RECORDED.items():
        for causal in (0, 1):
            got = _tb_sizes_and_plans(lib, norm, causal, dtype, _TB_SHAPES[i])
            assert got == want, (norm, causal, dtype, _TB_SHAPES[i], got)
    for (var, val), want in _TB_RECORDED_ENV.items():
        with monkeypatch.context() as mp:
            mp.setenv(var, val)
            got = _tb_sizes_and_plans(lib, 0, 0, 1, _TB_SHAPES[1])
        assert got == want, (var, val, got)


def test_pit_speaker_range(lib):
    """ctn_pit_workspace_bytes: 1..16 speakers (C <= 10 enumerated, 11..16 by assignment),
    0 bytes (unsupported) beyond."""
    import ctn_lib as L
    for C, ok in ((1, True), (8, True), (9, True), (16, True), (17, False)):
        n = lib.ctn_pit_workspace_bytes(ctypes.byref(L.PitDesc(4, C, 1000)))
        assert (n > 0) == ok, (C, n)


def test_mfma_peak_validation(lib):
    """ctn_mfma_peak (bench calibration microbenchmark) checks its arguments before launching."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.ctn_mfma_peak(0, 1, 1, None, None, None) == 1          # no output
    assert lib.ctn_mfma_peak(2, 1, 1, p, None, None) == 1             # unknown shape
    assert "shape" in lib.ctn_last_error().decode()
    assert lib.ctn_mfma_peak(0, 0, 1, p, None, None) == 1             # no workgroups
    assert lib.ctn_mfma_peak(1, 1, 0, p, None, None) == 1             # no iterations
