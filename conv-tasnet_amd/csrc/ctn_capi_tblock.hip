// C-ABI entries of the TemporalBlock (include/ctn.h ctn_tblock_*): gLN / cLN blocks driven
// by a per-call block plan (TbPlan), and BatchNorm1d blocks in identity-gLN mode.
#include <string>

#include "ctn_capi_util.h"

using namespace ctn;

static int tb_check(const ctn_tblock_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->K < 1 || d->Kp < d->K || d->Kp % 128)
    return fail(CTN_ERR_ARG, "bad frame geometry M=%d K=%d Kp=%d (Kp must be a multiple of 128 >= K)", d->M,
                d->K, d->Kp);
  if (d->B % 8 || d->H % 8 || d->B < 8 || d->H < 8)
    return fail(CTN_ERR_UNSUPPORTED, "B=%d H=%d must be multiples of 8", d->B, d->H);
  if (d->P < 1 || d->P > 8) return fail(CTN_ERR_UNSUPPORTED, "P=%d outside 1..8", d->P);
  if (!d->causal && d->P % 2 == 0)
    return fail(CTN_ERR_ARG, "non-causal padding (P-1)*d//2 needs odd P (conv_tasnet.py:236)");
  if (d->norm_type != CTN_NORM_GLN && d->norm_type != CTN_NORM_CLN && d->norm_type != CTN_NORM_BN)
    return fail(CTN_ERR_ARG, "norm_type %d", d->norm_type);
  {
    const int cg = d->H / 8;
    if (cg > 64 || (cg & (cg - 1))) return fail(CTN_ERR_UNSUPPORTED, "H=%d: need H/8 a power of two <= 64", d->H);
  }
  if (d->dtype != CTN_DTYPE_F32 && d->dtype != CTN_DTYPE_BF16) return fail(CTN_ERR_ARG, "dtype %d", d->dtype);
  if (d->dilation < 1) return fail(CTN_ERR_ARG, "dilation %d", d->dilation);
  return CTN_OK;
}

static int tb_groups(const ctn_tblock_desc* d) {
  if (d->norm_type == CTN_NORM_BN) return d->H;   // per-channel statistics
  return d->norm_type == CTN_NORM_GLN ? d->M : d->M * d->Kp;
}

extern "C" int ctn_tblock_stats_floats(const ctn_tblock_desc* d) { return 4 * tb_groups(d); }

namespace {
DType tb_dt(const ctn_tblock_desc* d) { return d->dtype == CTN_DTYPE_BF16 ? BF16 : F32; }

// ---------------------------------------------------------------------------
// Descriptor builders: every kernel descriptor of a block with everything but the data
// pointers filled in.  `norm` is the block's norm_type, or NORM_GLN for the BN path, whose
// kernels run in identity gLN mode.
// ---------------------------------------------------------------------------
DwArgs tb_dw(const ctn_tblock_desc* d, int norm, bool bwd) {
  DwArgs da{};
  da.g = Rows{d->M, d->K, d->Kp};
  da.H = d->H; da.P = d->P; da.dil = d->dilation; da.norm = norm;
  da.pad = d->causal ? (d->P - 1) * d->dilation : (d->P - 1) * d->dilation / 2;
  da.seg = dw_seg(da, bwd);   // the forward and the backward kernel have their own comb geometry
  return da;
}
// x[., B] -> [., H]: the forward 1x1 (EPI_PRELU_STATS; BN: EPI_STORE) and the backward
// g_n2 = gy . W2 (EPI_NORM_BWD, with the pre-activation d as R; BN: EPI_STORE)
GemmRows tb_gemm_in(const ctn_tblock_desc* d, int norm, int epi) {
  GemmRows g{};
  g.g = Rows{d->M, d->K, d->Kp};
  g.Kred = d->B; g.Nout = d->H; g.norm = norm;
  g.lda = d->B; g.ldw = d->B; g.ldc = d->H;
  g.epi = epi;
  if (epi == EPI_NORM_BWD) g.ldr = d->H;
  return g;
}
// op([., H]) -> [., B] + residual: the output 1x1 (op = norm 2 + PReLU), and the backward
// gx = op(g) . W1 + gy with op = the norm-1/PReLU-1 backward (fused path) or plain
GemmRows tb_gemm_out(const ctn_tblock_desc* d, int norm, int aop) {
  GemmRows g{};
  g.g = Rows{d->M, d->K, d->Kp};
  g.Kred = d->H; g.Nout = d->B; g.norm = norm;
  g.lda = d->H; g.ldw = d->H; g.epi = EPI_RESID; g.ldr = d->B; g.ldc = d->B;
  g.aop.kind = aop;
  if (aop != OP_PLAIN) g.aop.norm = norm;
  return g;
}
// dW2 = gy^T . norm2(PReLU(d)) and dW1 = gh1^T . x
GemmCols tb_cols2(const ctn_tblock_desc* d, int norm) {
  GemmCols c{};
  c.g = Rows{d->M, d->K, d->Kp};
  c.P = d->B; c.Q = d->H; c.lda = d->B; c.ldb = d->H;
  c.bop.kind = OP_PRELU_NORM; c.bop.norm = norm;
  return c;
}
GemmCols tb_cols1(const ctn_tblock_desc* d) {
  GemmCols c{};
  c.g = Rows{d->M, d->K, d->Kp};
  c.P = d->H; c.Q = d->B; c.lda = d->H; c.ldb = d->B;
  return c;
}
// The backward's dual GEMM (ctn_dual_ws.hip), shapes and operand ops only: pair A,
//   g_n2 = gy . W2 (norm-2 backward epilogue) + dW2 = gy^T . norm2(PReLU(d))
GemmDual tb_dualA(const ctn_tblock_desc* d) {
  GemmDual g{};
  g.g = Rows{d->M, d->K, d->Kp};
  g.Kred = d->B; g.Nout = d->H; g.norm = d->norm_type;
  g.lda = d->B; g.ldw = d->B; g.ldc = d->H; g.ldr = d->H; g.ldb = d->H;
  g.epi = EPI_NORM_BWD;
  g.bop.kind = OP_PRELU_NORM; g.bop.norm = d->norm_type;
  return g;
}

// gLN statistics of the weight-stationary GEMMs' operands: folded from the producer's
// partials in every workgroup's prologue (default) or finalized by a separate launch
// before them (A/B; read on every call).  bit 0: the output 1x1 GEMM (norm 2 from dw_fwd),
// bit 1: the gx GEMM (norm-1 backward sums from dw_bwd).
int ws_fold_mask() {
  const char* e = getenv("CTN_WS_FOLD");
  return e ? atoi(e) : 3;
}

// ---------------------------------------------------------------------------
// The block plan: everything about a gLN / cLN block that does not depend on data pointers,
// computed once per call from the descriptor (and the A/B environment switches, which is
// why it is never cached across calls).  The workspace carve, the launch sequences, the
// gradient reductions and ctn_tblock_plan all read this one copy, so a slab is sized by the
// very descriptor and decision its launch uses.  Only the direction asked for is filled in
// (a call runs one), except the depthwise geometry, which both directions carry.
// ---------------------------------------------------------------------------
struct TbPlan {
  Rows rg;
  DType dt;
  int B, H, P;
  int G;        // statistics groups: utterances (gLN) or frame rows (cLN)
  double cnt;   // elements per group
  bool fold;    // gLN: the consumers finalize statistics from slab partials (StatFold)
  DwArgs dwF, dwB;
  // forward
  GemmRows g1, g2;    // 1x1 B->H with PReLU statistics; norm 2 + PReLU, 1x1 H->B, residual
  bool fin1;          // cLN: the WS kernel of g1 writes the final per-row statistics
  bool fold2;         // gLN: g2 folds the norm-2 statistics itself (CTN_WS_FOLD bit 0)
  StatFold f_st1;     // gLN: norm-1 statistics fold of dw_fwd over g1's partials
  int parts1, parts2; // slab parts per group of g1 / dw_fwd
  // backward
  GemmRows ga, gbF, gbP;   // pair A's row GEMM; gx GEMM, fused (norm-1 backward operand) / plain
  GemmDual duA;
  GemmCols c1, c2;         // dW1, dW2
  bool dualA;              // pair A runs as one dual GEMM
  bool fused1;             // norm-1/PReLU-1 backward inside gbF; else norm1_bwd_kernel
  bool foldX;              // fused1, gLN: gbF folds the norm-1 sums itself (CTN_WS_FOLD bit 1)
  bool clnFoldA;           // cLN: the wave-item dw_bwd folds the dual's per-row partials itself
  StatFold f_sm2;          // norm-2 backward sums fold of dw_bwd over pair A's partials
  int partsA, partsD;      // slab parts per group of pair A / dw_bwd
  int chunks1, chunks2;    // dW1 / dW2 partials
  int dwb, dws, ewb;       // dw_bwd workgroups, their column-partial stride, norm1_bwd blocks
  int nalpha;              // alpha-1 gradient partials

  // The kernel a launcher will pick by itself for one of the plan's descriptors, for
  // ctn_tblock_plan: the launcher's own eligibility function on the descriptor the launch
  // copies.  Asked only there, so that a forward or backward call pays for no query it does
  // not act on.
  const char* rows_kernel(const GemmRows& g) const { return gemm_ws_eligible(dt, g) ? "ws" : "rows"; }
  const char* dw_kernel(bool bwd) const { return dw_wave_eligible(dt, bwd ? dwB : dwF) ? "wave" : "lane"; }
};

TbPlan tb_plan(const ctn_tblock_desc* d, bool backward) {
  TbPlan pl{};
  const int nk = d->norm_type;
  const DType dt = pl.dt = tb_dt(d);
  pl.rg = Rows{d->M, d->K, d->Kp};
  pl.B = d->B; pl.H = d->H; pl.P = d->P;
  pl.G = tb_groups(d);
  pl.fold = nk == CTN_NORM_GLN;
  pl.cnt = pl.fold ? (double)d->K * d->H : (double)d->H;
  pl.dwF = tb_dw(d, nk, false);
  pl.dwB = tb_dw(d, nk, true);
  if (!backward) {
    pl.g1 = tb_gemm_in(d, nk, EPI_PRELU_STATS);
    pl.g2 = tb_gemm_out(d, nk, OP_PRELU_NORM);
    // cLN on the WS kernel: the workgroup holds all H channels of its rows and writes
    // the final per-row statistics itself; the depthwise kernel does the same for norm 2
    pl.fin1 = !pl.fold && gemm_ws_final_cln(dt, pl.g1);
    if (pl.fin1) pl.g1.eps = (float)kEps;
    if (!pl.fold) pl.dwF.eps = (float)kEps;
    if (pl.fold) {
      pl.f_st1 = gemm_rows_stat_fold(dt, pl.g1, nullptr, pl.cnt, (float)kEps, 0, nullptr);
      pl.parts1 = pl.f_st1.parts;
    } else {
      pl.parts1 = gemm_rows_tiles_per_group(dt, pl.g1);
    }
    pl.parts2 = dw_parts_per_group(pl.dwF);
    pl.fold2 = pl.fold && (ws_fold_mask() & 1) && gemm_ws_can_fold(dt, pl.g2);
    return pl;
  }
  pl.ga = tb_gemm_in(d, nk, EPI_NORM_BWD);
  pl.gbF = tb_gemm_out(d, nk, OP_NORM1_BWD);
  pl.gbP = tb_gemm_out(d, nk, OP_PLAIN);
  pl.duA = tb_dualA(d);
  pl.c1 = tb_cols1(d);
  pl.c2 = tb_cols2(d, nk);
  // Some eligibility functions of the kernel files also look at operand pointers, which a
  // plan does not have.  Left null they answer as at the launch: pair A wants one statistics
  // table for both of its uses (the launch passes st2 twice).  Only the norm-1-backward
  // operand of gbF must be present to be eligible; the launch always supplies all of it, so
  // the query below gets a stand-in for every pointer it tests.
  pl.dualA = gemm_dual_eligible(dt, pl.duA);
  // The norm-1/PReLU-1 backward runs inside the first 1x1's two gradient GEMMs (bf16,
  // weight-stationary data-gradient kernel); else norm1_bwd_kernel.
  // CTN_FUSE_N1=0 keeps the separate kernel (read on every call, so a process can compare
  // both paths: tests/test_gpu_tblock.py).
  const char* fuse = getenv("CTN_FUSE_N1");
  if (!(fuse && atoi(fuse) == 0) && dt == BF16) {
    static const float there[2] = {0.f, 0.f};
    GemmRows q = pl.gbF;
    q.aop.aux = there; q.aop.apart = const_cast<float*>(there); q.aop.aout = const_cast<float*>(there);
    q.aop.stats = q.aop.sums = reinterpret_cast<const float2*>(there);
    pl.fused1 = gemm_ws_eligible(BF16, q);
  }
  pl.foldX = pl.fused1 && pl.fold && (ws_fold_mask() & 2);
  pl.partsD = dw_parts_per_group(pl.dwB);
  pl.chunks2 = pl.dualA ? gemm_dual_ranges(pl.duA) : gemm_cols_chunks(pl.c2);
  pl.chunks1 = gemm_cols_chunks(pl.c1);
  pl.dwb = dw_blocks(pl.dwB);
  pl.dws = dw_col_stride(pl.dwB);
  pl.ewb = ew_blocks(pl.dwB);
  pl.nalpha = pl.fused1 ? gemm_ws_grid(pl.gbF) : pl.ewb;
  // The norm-2 backward sums reach dw_bwd as pair A's partials.  gLN: always folded there.
  // cLN: the wave-item depthwise backward folds the dual's per-row partials itself (at most
  // 4 per row: one per 128-channel slice); otherwise a finalize launch makes them final.
  if (pl.fold) {
    pl.f_sm2 = pl.dualA ? gemm_dual_stat_fold(pl.duA, nullptr, pl.cnt, 0.f, 1, nullptr)
                        : gemm_rows_stat_fold(dt, pl.ga, nullptr, pl.cnt, 0.f, 1, nullptr);
    pl.partsA = pl.f_sm2.parts;
  } else {
    pl.partsA = pl.dualA ? gemm_dual_group_parts(pl.duA) : gemm_rows_tiles_per_group(dt, pl.ga);
    pl.clnFoldA = pl.dualA && pl.partsA <= 4 && dw_wave_eligible(dt, pl.dwB);
    if (pl.clnFoldA) pl.f_sm2 = gemm_dual_stat_fold(pl.duA, nullptr, pl.cnt, 0.f, 1, nullptr);
  }
  return pl;
}

struct TbLayout {
  // forward
  void *w1s, *w2s;
  double2 *slab1, *slab2;
  // backward
  void *w1t, *w2t, *G1, *G2;
  double2 *slabA, *slabD;
  float *colD, *alphaSlab, *cpart1, *cpart2, *srtmp;
  float2 *sums1, *sums2;
  size_t bytes;
  size_t part_bytes;   // split_parts: the parameter-gradient partials' own buffer
};

// backward, split_parts: the parameter-gradient partials (colD, alphaSlab, cpart1/2) and
// their reduction scratch (srtmp) come from `part` (part_bytes), everything else from ws
// (bytes) — the deferred backward (ctn_tblock_backward_deferred) keeps only `part` alive
// until ctn_tblock_reduce_grads.
TbLayout tb_layout(const TbPlan& pl, int backward, void* ws, void* part = nullptr, bool split_parts = false) {
  TbLayout L{};
  Carver c(ws), cpt(part);
  Carver& cp = split_parts ? cpt : c;
  const size_t es = pl.dt == BF16 ? 2 : 4;
  const size_t HB = (size_t)pl.H * pl.B, rows = (size_t)pl.rg.rows(), G = (size_t)pl.G;
  if (!backward) {
    if (pl.dt == BF16) {
      L.w1s = c.take<void>(HB * es);
      L.w2s = c.take<void>(HB * es);
    }
    L.slab1 = c.take<double2>(G * pl.parts1 * sizeof(double2));
    L.slab2 = c.take<double2>(G * pl.parts2 * sizeof(double2));
  } else {
    L.w1t = c.take<void>(HB * es);
    L.w2t = c.take<void>(HB * es);
    L.G1 = c.take<void>(rows * pl.H * es);
    L.G2 = c.take<void>(rows * pl.H * es);
    L.slabA = c.take<double2>(G * pl.partsA * sizeof(double2));
    L.slabD = c.take<double2>(G * pl.partsD * sizeof(double2));
    L.colD = cp.take<float>((size_t)pl.dwb * pl.dws * sizeof(float));
    L.alphaSlab = cp.take<float>((size_t)(pl.nalpha > pl.ewb ? pl.nalpha : pl.ewb) * sizeof(float));
    L.sums1 = c.take<float2>(G * sizeof(float2));
    L.sums2 = c.take<float2>(G * sizeof(float2));
    L.cpart2 = cp.take<float>(pl.chunks2 * HB * sizeof(float));
    L.cpart1 = cp.take<float>(pl.chunks1 * HB * sizeof(float));
    const size_t ntmp = sr_tmp(pl.chunks2, HB) + sr_tmp(pl.chunks1, HB) + 4 * sr_tmp(pl.dwb, pl.H) +
                        sr_tmp(pl.dwb, (long)pl.H * pl.P) + sr_tmp(pl.dwb, 1) + sr_tmp(pl.ewb, 1);
    L.srtmp = cp.take<float>(ntmp * sizeof(float));
  }
  L.bytes = c.off + 256;
  L.part_bytes = split_parts ? cpt.off + 256 : 0;
  return L;
}

// The 1x1 weights in the storage type, and for the backward transposed: the caller's bf16
// copies with their fragment-ordered companions (ctn_pack_weights, once per step), or
// copies made by this call into s1 / s2 (W1's and W2's workspace slots).
struct TbWeights {
  const void *w1, *w2;     // backward: the transposes
  const void *w1f, *w2f;   // fragment order (caller packs only), else null
};
int tb_weights(DType dt, const ctn_tblock_desc* d, const ctn_tblock_params* p, bool backward, void* s1, void* s2,
               hipStream_t s, TbWeights* w) {
  const void* c1 = backward ? p->w1t_bf16 : p->w1_bf16;
  const void* c2 = backward ? p->w2t_bf16 : p->w2_bf16;
  if (dt == BF16 && c1 && c2) {
    *w = backward ? TbWeights{c1, c2, p->w1t_frag, p->w2t_frag} : TbWeights{c1, c2, p->w1_frag, p->w2_frag};
    return CTN_OK;
  }
  if (!backward && dt != BF16) {   // the fp32 forward reads the parameters as they are
    *w = TbWeights{p->w1, p->w2, nullptr, nullptr};
    return CTN_OK;
  }
  PrepBatch pb{};
  if (backward) {
    pb.d[0] = PrepDesc{p->w2, d->B, d->H, nullptr, s2};   // [H][B]
    pb.d[1] = PrepDesc{p->w1, d->H, d->B, nullptr, s1};   // [B][H]
  } else {
    pb.d[0] = PrepDesc{p->w1, d->H, d->B, s1, nullptr};
    pb.d[1] = PrepDesc{p->w2, d->B, d->H, s2, nullptr};
  }
  pb.nd = 2;
  CTN_HIP(launch_prep_weights(dt, pb, s));
  *w = TbWeights{s1, s2, nullptr, nullptr};
  return CTN_OK;
}

// ===========================================================================
// TemporalBlock with BatchNorm1d norms (norm_type "BN", conv_tasnet.py:302-303)
// ===========================================================================
// The block's kernels run in identity gLN mode (per-utterance stats (0, 1),
// gamma' = gamma*rstd, beta' = beta - gamma*mean*rstd per channel, ctn_bn.hip);
// BN's per-channel statistics and the per-channel mean subtractions of its
// backward run in the column kernels of ctn_bn.hip.
struct BnLayout {
  void *w1s, *w2s, *w1t, *w2t, *G1, *G2;
  double2 *part, *slab2, *slabD;
  float2 *ident, *zero, *sums1, *sums2;
  float *ge1, *be1, *ge2, *be2, *colD, *alphaSlab, *cpart1, *cpart2, *srtmp;
  int chunks1, chunks2;
  size_t bytes;
};
BnLayout bn_layout(const ctn_tblock_desc* d, int backward, void* ws) {
  BnLayout L{};
  Carver c(ws);
  const Rows rg{d->M, d->K, d->Kp};
  const long rows = rg.rows();
  const size_t es = esize(d->dtype);
  const int H = d->H, B = d->B, M = d->M, nb = bn_blocks(rg);
  L.part = c.take<double2>((size_t)nb * H * sizeof(double2));
  L.ident = c.take<float2>((size_t)M * sizeof(float2));
  L.zero = c.take<float2>((size_t)M * sizeof(float2));
  L.ge1 = c.take<float>((size_t)H * sizeof(float));
  L.be1 = c.take<float>((size_t)H * sizeof(float));
  L.ge2 = c.take<float>((size_t)H * sizeof(float));
  L.be2 = c.take<float>((size_t)H * sizeof(float));
  if (!backward) {
    if (d->dtype == CTN_DTYPE_BF16) {
      L.w1s = c.take<void>((size_t)H * B * es);
      L.w2s = c.take<void>((size_t)H * B * es);
    }
    const DwArgs da = tb_dw(d, NORM_GLN, false);
    L.slab2 = c.take<double2>((size_t)M * dw_parts_per_group(da) * sizeof(double2));
  } else {
    L.w1t = c.take<void>((size_t)H * B * es);
    L.w2t = c.take<void>((size_t)H * B * es);
    L.G1 = c.take<void>((size_t)rows * H * es);
    L.G2 = c.take<void>((size_t)rows * H * es);
    L.sums1 = c.take<float2>((size_t)H * sizeof(float2));
    L.sums2 = c.take<float2>((size_t)H * sizeof(float2));
    const DwArgs da = tb_dw(d, NORM_GLN, true);
    L.slabD = c.take<double2>((size_t)M * dw_parts_per_group(da) * sizeof(double2));
    L.colD = c.take<float>((size_t)dw_blocks(da) * dw_col_stride(da) * sizeof(float));
    L.alphaSlab = c.take<float>((size_t)nb * sizeof(float));
    L.chunks2 = gemm_cols_chunks(tb_cols2(d, NORM_GLN));
    L.cpart2 = c.take<float>((size_t)L.chunks2 * B * H * sizeof(float));
    L.chunks1 = gemm_cols_chunks(tb_cols1(d));
    L.cpart1 = c.take<float>((size_t)L.chunks1 * B * H * sizeof(float));
    const long HB = (long)H * B, dwb = dw_blocks(da);
    const size_t ntmp = sr_tmp(L.chunks2, HB) + sr_tmp(L.chunks1, HB) + 2 * sr_tmp(dwb, H) +
                        sr_tmp(dwb, (long)H * d->P) + sr_tmp(dwb, 1) + sr_tmp(nb, 1);
    L.srtmp = c.take<float>(ntmp * sizeof(float));
  }
  L.bytes = c.off + 256;
  return L;
}

// forward statistics of PReLU(a) -> stats, gamma', beta', running statistics
int bn_forward_stats(DType dt, const ctn_tblock_desc* d, const BnLayout& L, const void* a, const float* alpha,
                     const float* gamma, const float* beta, float* rmean, float* rvar, int training, float mom,
                     float eps, float2* stats, float* ge, float* be, hipStream_t s) {
  const Rows rg{d->M, d->K, d->Kp};
  const bool batch = training || !rmean;
  if (!batch && !rvar) return fail(CTN_ERR_ARG, "BN eval mode needs running_var");
  if (batch) {
    BnArgs ba{};
    ba.g = rg; ba.H = d->H; ba.a = a; ba.alpha = alpha; ba.part = L.part;
    CTN_HIP(launch_bn_partials(dt, ba, 0, s));
  }
  BnFinal bf{};
  bf.H = d->H; bf.M = d->M; bf.nparts = bn_blocks(rg); bf.count = (long)d->M * d->K; bf.part = L.part;
  bf.training = batch; bf.momentum = mom; bf.eps = eps;
  bf.run_mean = training ? rmean : (batch ? nullptr : rmean);
  bf.run_var = training ? rvar : (batch ? nullptr : rvar);
  bf.gamma = gamma; bf.beta = beta; bf.stats = stats; bf.gamma_eff = ge; bf.beta_eff = be;
  bf.ident = L.ident; bf.zero = L.zero;
  CTN_HIP(launch_bn_finalize(bf, 0, s));
  return CTN_OK;
}
}  // namespace

static int tb_forward_bn(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x, void* y,
                         const ctn_tblock_saved* sv, void* ws, size_t ws_bytes, hipStream_t s) {
  const BnLayout L = bn_layout(d, 0, ws);
  if (!ws || ws_bytes < L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, L.bytes);
  const DType dt = tb_dt(d);
  float2* st1 = reinterpret_cast<float2*>(sv->stats);
  float2* st2 = st1 + d->H;
  TbWeights w;
  int rc = tb_weights(dt, d, p, false, L.w1s, L.w2s, s, &w);
  if (rc) return rc;
  // 1x1 conv B->H (pre-PReLU h1)
  GemmRows g1 = tb_gemm_in(d, NORM_GLN, EPI_STORE);
  g1.A = x; g1.W = w.w1; g1.C = sv->h1;
  CTN_HIP(launch_gemm_rows(dt, g1, s));
  // BN-1 statistics of PReLU(h1)
  rc = bn_forward_stats(dt, d, L, sv->h1, p->alpha1, p->gamma1, p->beta1, p->bn_mean1, p->bn_var1,
                        p->bn_training, p->bn_momentum1, p->bn_eps1, st1, L.ge1, L.be1, s);
  if (rc) return rc;
  // BN-1 apply (identity gLN) + dilated depthwise conv
  DwArgs da = tb_dw(d, NORM_GLN, false);
  da.h1 = sv->h1; da.st1 = L.ident;
  da.alpha1 = p->alpha1; da.gamma1 = L.ge1; da.beta1 = L.be1; da.alpha2 = p->alpha2;
  da.wd = p->wd; da.d_out = sv->d; da.slab2 = L.slab2;
  CTN_HIP(launch_dw_fwd(dt, da, s));
  // BN-2 statistics of PReLU(d)
  rc = bn_forward_stats(dt, d, L, sv->d, p->alpha2, p->gamma2, p->beta2, p->bn_mean2, p->bn_var2,
                        p->bn_training, p->bn_momentum2, p->bn_eps2, st2, L.ge2, L.be2, s);
  if (rc) return rc;
  // BN-2 apply (identity gLN, with PReLU) on the operand, 1x1 conv H->B, residual
  GemmRows g2 = tb_gemm_out(d, NORM_GLN, OP_PRELU_NORM);
  g2.A = sv->d; g2.W = w.w2; g2.R = x; g2.C = y;
  g2.aop.stats = L.ident; g2.aop.gamma = L.ge2; g2.aop.beta = L.be2; g2.aop.alpha = p->alpha2;
  CTN_HIP(launch_gemm_rows(dt, g2, s));
  return CTN_OK;
}

static int tb_backward_bn(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                          const ctn_tblock_saved* sv, const void* gy, void* gx, const ctn_tblock_grads* gr, void* ws,
                          size_t ws_bytes, hipStream_t s) {
  const BnLayout L = bn_layout(d, 1, ws);
  if (!ws || ws_bytes < L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, L.bytes);
  const DType dt = tb_dt(d);
  const Rows rg{d->M, d->K, d->Kp};
  const int H = d->H, nb = bn_blocks(rg);
  const float2* st1 = reinterpret_cast<const float2*>(sv->stats);
  const float2* st2 = st1 + H;
  const int train1 = p->bn_training || !p->bn_mean1, train2 = p->bn_training || !p->bn_mean2;
  TbWeights w;
  if (int rc = tb_weights(dt, d, p, true, L.w1t, L.w2t, s, &w)) return rc;
  // gamma' / beta' from the saved statistics; identity and zero tables
  {
    BnFinal pf{};
    pf.H = H; pf.M = d->M; pf.gamma = p->gamma1; pf.beta = p->beta1; pf.stats = const_cast<float2*>(st1);
    pf.gamma_eff = L.ge1; pf.beta_eff = L.be1; pf.ident = L.ident; pf.zero = L.zero;
    CTN_HIP(launch_bn_finalize(pf, 2, s));
    pf.gamma = p->gamma2; pf.beta = p->beta2; pf.stats = const_cast<float2*>(st2);
    pf.gamma_eff = L.ge2; pf.beta_eff = L.be2; pf.ident = nullptr; pf.zero = nullptr;
    CTN_HIP(launch_bn_finalize(pf, 2, s));
  }
  // (a) G1 = dL/dn2 = gy . W2
  GemmRows ga = tb_gemm_in(d, NORM_GLN, EPI_STORE);
  ga.A = gy; ga.W = w.w2; ga.C = L.G1;
  CTN_HIP(launch_gemm_rows(dt, ga, s));
  // (b) dW2 partials = gy^T . BN2(PReLU(d))
  GemmCols c2 = tb_cols2(d, NORM_GLN);
  c2.A = gy; c2.B = sv->d;
  c2.bop.stats = L.ident; c2.bop.gamma = L.ge2; c2.bop.beta = L.be2; c2.bop.alpha = p->alpha2;
  c2.Cpart = L.cpart2; c2.nchunks = L.chunks2;
  CTN_HIP(launch_gemm_cols(dt, c2, s));
  // (c) BN-2 backward sums (= beta2 / gamma2 gradients) and (d) G1 -= per-channel means
  BnArgs ba{};
  ba.g = rg; ba.H = H; ba.part = L.part;
  ba.a = sv->d; ba.gin = L.G1; ba.gout = L.G1; ba.alpha = p->alpha2; ba.stats = st2; ba.sums = L.sums2;
  CTN_HIP(launch_bn_partials(dt, ba, 1, s));
  BnFinal bf{};
  bf.H = H; bf.M = d->M; bf.nparts = nb; bf.count = (long)d->M * d->K; bf.part = L.part;
  bf.training = train2; bf.sums = L.sums2; bf.dgamma = gr->gamma2; bf.dbeta = gr->beta2;
  CTN_HIP(launch_bn_finalize(bf, 1, s));
  CTN_HIP(launch_bn_apply(dt, ba, false, s));
  // (e) depthwise backward in identity mode -> G2 = dL/dn1 * gamma1' ; wd, alpha2 and
  //     (gamma1', beta1') column partials
  DwArgs da = tb_dw(d, NORM_GLN, true);
  da.h1 = sv->h1; da.d = sv->d; da.st1 = L.ident; da.st2 = L.ident;
  da.alpha1 = p->alpha1; da.gamma1 = L.ge1; da.beta1 = L.be1; da.alpha2 = p->alpha2; da.gamma2 = L.ge2;
  da.wd = p->wd;
  da.ga2 = L.G1; da.sm2 = L.zero; da.ga1_out = L.G2; da.slab1 = L.slabD; da.col_slab = L.colD;
  CTN_HIP(launch_dw_bwd(dt, da, s));
  // (f) BN-1 backward sums over (G2, h1), (g) G1 = (G2 - means) * PReLU'(h1), alpha-1 partials
  ba.a = sv->h1; ba.gin = L.G2; ba.gout = L.G1; ba.alpha = p->alpha1; ba.stats = st1; ba.sums = L.sums1;
  ba.apart = L.alphaSlab;
  CTN_HIP(launch_bn_partials(dt, ba, 1, s));
  bf.training = train1; bf.sums = L.sums1; bf.dgamma = nullptr; bf.dbeta = nullptr;
  CTN_HIP(launch_bn_finalize(bf, 1, s));
  CTN_HIP(launch_bn_apply(dt, ba, true, s));
  // (h) gx = G1 . W1 + gy ; dW1 partials = G1^T . x
  GemmRows gb = tb_gemm_out(d, NORM_GLN, OP_PLAIN);
  gb.A = L.G1; gb.W = w.w1; gb.R = gy; gb.C = gx;
  CTN_HIP(launch_gemm_rows(dt, gb, s));
  GemmCols c1 = tb_cols1(d);
  c1.A = L.G1; c1.B = x; c1.Cpart = L.cpart1; c1.nchunks = L.chunks1;
  CTN_HIP(launch_gemm_cols(dt, c1, s));
  // (i) parameter-gradient partial sums, (j) gamma1 from the identity-mode (gamma1', beta1')
  const int dwb = dw_blocks(da), dws = dw_col_stride(da);
  const int HB = H * d->B;
  SlabBatch sb{};
  sb.d[0] = SlabDesc{L.cpart2, gr->w2, L.chunks2, HB, HB};
  sb.d[1] = SlabDesc{L.cpart1, gr->w1, L.chunks1, HB, HB};
  sb.d[2] = SlabDesc{L.colD + dw_col_off_gamma1(d->P, H), gr->gamma1, dwb, H, dws};
  sb.d[3] = SlabDesc{L.colD + dw_col_off_beta1(d->P, H), gr->beta1, dwb, H, dws};
  sb.d[4] = SlabDesc{L.colD + dw_col_off_wd(d->P, H), gr->wd, dwb, H * d->P, dws};
  sb.d[5] = SlabDesc{L.colD + dw_col_off_alpha2(d->P, H), gr->alpha2, dwb, 1, dws};
  sb.d[6] = SlabDesc{L.alphaSlab, gr->alpha1, nb, 1, 1};
  sb.nd = 7;
  CTN_HIP(launch_slab_reduce(sb, L.srtmp, s));
  CTN_HIP(launch_bn_gamma_fix(gr->gamma1, gr->beta1, st1, H, s));
  return CTN_OK;
}

// ===========================================================================
// gLN / cLN blocks
// ===========================================================================
extern "C" size_t ctn_tblock_workspace_bytes(const ctn_tblock_desc* d, int backward) {
  if (tb_check(d) != CTN_OK) return 0;
  if (d->norm_type == CTN_NORM_BN) return bn_layout(d, backward, nullptr).bytes;
  return tb_layout(tb_plan(d, backward), backward, nullptr).bytes;
}

extern "C" int ctn_tblock_forward(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x, void* y,
                                  const ctn_tblock_saved* sv, void* ws, size_t ws_bytes, void* stream) {
  int rc = tb_check(d);
  if (rc) return rc;
  if (!p || !x || !y || !sv || !sv->h1 || !sv->d || !sv->stats) return fail(CTN_ERR_ARG, "null pointer");
  if (d->norm_type == CTN_NORM_BN) return tb_forward_bn(d, p, x, y, sv, ws, ws_bytes, (hipStream_t)stream);
  const TbPlan pl = tb_plan(d, false);
  const TbLayout L = tb_layout(pl, 0, ws);
  if (!ws || ws_bytes < L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, L.bytes);
  hipStream_t s = (hipStream_t)stream;
  const DType dt = pl.dt;
  float2* st1 = reinterpret_cast<float2*>(sv->stats);
  float2* st2 = st1 + pl.G;
  TbWeights w;
  if ((rc = tb_weights(dt, d, p, false, L.w1s, L.w2s, s, &w))) return rc;
  // 1x1 conv B->H, PReLU statistics for norm1
  GemmRows g1 = pl.g1;
  g1.A = x;
  g1.W = w.w1;
  g1.Wf = w.w1f;
  g1.alpha = p->alpha1;
  g1.C = sv->h1;
  g1.grp_slab = L.slab1;
  if (pl.fin1) g1.stats_out = st1;
  {
    TimedScope ts(CTN_TIMER_GEMM1, s);
    CTN_HIP(launch_gemm_rows(dt, g1, s));
  }
  // gLN: the consumers finalize the statistics from the slab partials (StatFold)
  if (!pl.fold && !pl.fin1)
    CTN_HIP(launch_stats_finalize(L.slab1, pl.G, pl.parts1, pl.cnt, 0, (float)kEps, st1, s));
  // norm1 apply + depthwise dilated conv, PReLU statistics for norm2
  DwArgs da = pl.dwF;
  da.h1 = sv->h1; da.st1 = st1;
  da.alpha1 = p->alpha1; da.gamma1 = p->gamma1; da.beta1 = p->beta1; da.alpha2 = p->alpha2;
  da.wd = p->wd; da.d_out = sv->d; da.slab2 = L.slab2;
  if (pl.fold) {
    da.f_st1 = pl.f_st1;
    da.f_st1.slab = L.slab1;
    da.f_st1.out = st1;
  } else {
    da.st2_out = st2;   // cLN: per-row statistics final in the depthwise kernel
  }
  {
    TimedScope ts(CTN_TIMER_DW_FWD, s);
    CTN_HIP(launch_dw_fwd(dt, da, s));
  }
  // norm2 apply (+PReLU) on the operand, 1x1 conv H->B, residual add
  GemmRows g2 = pl.g2;
  g2.A = sv->d;
  g2.aop.stats = st2; g2.aop.gamma = p->gamma2; g2.aop.beta = p->beta2; g2.aop.alpha = p->alpha2;
  g2.W = w.w2; g2.Wf = w.w2f;
  g2.R = x;
  g2.C = y;
  if (pl.fold2)
    g2.aop.fold = StatFold{L.slab2, pl.parts2, pl.cnt, (float)kEps, 0, st2};
  else if (pl.fold)
    CTN_HIP(launch_stats_finalize(L.slab2, pl.G, pl.parts2, pl.cnt, 0, (float)kEps, st2, s));
  {
    TimedScope ts(CTN_TIMER_GEMM2, s);
    CTN_HIP(launch_gemm_rows(dt, g2, s));
  }
  return CTN_OK;
}

// one fork event per device (hipStreamWaitEvent takes the event's state when it is
// called, so re-recording it for the next call is safe)
static hipError_t fork_stream(hipStream_t from, hipStream_t to) {
  static hipEvent_t ev[64] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  if (!ev[dev] && (e = hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming)) != hipSuccess) return e;
  if ((e = hipEventRecord(ev[dev], from)) != hipSuccess) return e;
  return hipStreamWaitEvent(to, ev[dev], 0);
}

// The fixed-order reductions of every parameter gradient of a block backward (step (g)):
// descriptors over the partials that layout L points at, into the gradients gr.
static int tb_grad_slabs(const TbPlan& pl, const TbLayout& L, const ctn_tblock_grads* gr, SlabDesc* out) {
  const int dwb = pl.dwb, dws = pl.dws;
  const int HB = pl.H * pl.B, H = pl.H, P = pl.P;
  out[0] = SlabDesc{L.cpart2, gr->w2, pl.chunks2, HB, HB};
  out[1] = SlabDesc{L.cpart1, gr->w1, pl.chunks1, HB, HB};
  out[2] = SlabDesc{L.colD + dw_col_off_gamma2(P, H), gr->gamma2, dwb, H, dws};
  out[3] = SlabDesc{L.colD + dw_col_off_beta2(P, H), gr->beta2, dwb, H, dws};
  out[4] = SlabDesc{L.colD + dw_col_off_gamma1(P, H), gr->gamma1, dwb, H, dws};
  out[5] = SlabDesc{L.colD + dw_col_off_beta1(P, H), gr->beta1, dwb, H, dws};
  out[6] = SlabDesc{L.colD + dw_col_off_wd(P, H), gr->wd, dwb, H * P, dws};
  out[7] = SlabDesc{L.colD + dw_col_off_alpha2(P, H), gr->alpha2, dwb, 1, dws};
  out[8] = SlabDesc{L.alphaSlab, gr->alpha1, pl.nalpha, 1, 1};
  return 9;
}

// sw: the stream of the parameter-gradient tail (== s: one stream).
// defer: the parameter-gradient partials go to `part` and step (g) is left to
// ctn_tblock_reduce_grads.
static int tb_backward(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                       const ctn_tblock_saved* sv, const void* gy, void* gx, const ctn_tblock_grads* gr,
                       void* ws, size_t ws_bytes, hipStream_t s, hipStream_t sw, void* part = nullptr,
                       size_t part_bytes = 0, bool defer = false) {
  int rc = tb_check(d);
  if (rc) return rc;
  if (!p || !x || !sv || !gy || !gx || !gr) return fail(CTN_ERR_ARG, "null pointer");
  if (d->norm_type == CTN_NORM_BN) {
    if (defer) return fail(CTN_ERR_UNSUPPORTED, "deferred gradient reductions: gLN / cLN blocks only");
    return tb_backward_bn(d, p, x, sv, gy, gx, gr, ws, ws_bytes, s);
  }
  const TbPlan pl = tb_plan(d, true);
  const TbLayout L = tb_layout(pl, 1, ws, part, defer);
  if (!ws || ws_bytes < L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, L.bytes);
  if (defer && (!part || part_bytes < L.part_bytes))
    return fail(CTN_ERR_WORKSPACE, "partials buffer %zu < %zu", part_bytes, L.part_bytes);
  const DType dt = pl.dt;
  const float2* st1 = reinterpret_cast<const float2*>(sv->stats);
  const float2* st2 = st1 + pl.G;
  TbWeights w;   // the transposes
  if ((rc = tb_weights(dt, d, p, true, L.w1t, L.w2t, s, &w))) return rc;

  // (a) G1 = g_n2 = gy . W2 ; epilogue: norm-2 backward sums of (g_n2*gamma2, g_n2*gamma2*hat a2)
  // (b) dW2 = gy^T . norm2(PReLU(d))            — one dual-GEMM pass when eligible
  if (pl.dualA) {
    GemmDual duA = pl.duA;
    duA.A = gy; duA.W = w.w2; duA.Wf = w.w2f; duA.R = sv->d; duA.C = L.G1;
    duA.alpha = p->alpha2; duA.stats = st2; duA.gamma = p->gamma2; duA.grp_slab = L.slabA;
    duA.Bm = sv->d;
    duA.bop.stats = st2; duA.bop.gamma = p->gamma2; duA.bop.beta = p->beta2; duA.bop.alpha = p->alpha2;
    duA.Dpart = L.cpart2;
    TimedScope ts(CTN_TIMER_GEMM_A, s);
    CTN_HIP(launch_gemm_dual(duA, s));
  } else {
    GemmRows ga = pl.ga;
    ga.A = gy;
    ga.W = w.w2;
    ga.Wf = w.w2f;
    ga.R = sv->d;
    ga.alpha = p->alpha2; ga.stats = st2; ga.gamma = p->gamma2;
    ga.C = L.G1;
    ga.grp_slab = L.slabA;
    {
      TimedScope ts(CTN_TIMER_GEMM_A, s);
      CTN_HIP(launch_gemm_rows(dt, ga, s));
    }
    GemmCols c2 = pl.c2;
    c2.A = gy; c2.B = sv->d;
    c2.bop.stats = st2; c2.bop.gamma = p->gamma2; c2.bop.beta = p->beta2; c2.bop.alpha = p->alpha2;
    c2.Cpart = L.cpart2; c2.nchunks = pl.chunks2;
    CTN_HIP(launch_gemm_cols(dt, c2, s));
  }

  // (c) depthwise backward -> G2 = dL/d(hat a1), norm1 sums, column partials (gamma1/beta1,
  //     wd, gamma2/beta2, alpha2)
  DwArgs da = pl.dwB;
  da.h1 = sv->h1; da.d = sv->d; da.st1 = st1; da.st2 = st2;
  da.alpha1 = p->alpha1; da.gamma1 = p->gamma1; da.beta1 = p->beta1; da.alpha2 = p->alpha2; da.gamma2 = p->gamma2;
  da.wd = p->wd;
  da.ga2 = L.G1; da.sm2 = L.sums2; da.ga1_out = L.G2; da.slab1 = L.slabD; da.col_slab = L.colD;
  if (!pl.fold) da.sm1_out = L.sums1;   // cLN: per-row norm-1 backward means final in the depthwise kernel
  if (pl.fold || pl.clnFoldA) {         // norm-2 backward sums folded from pair A's partials
    da.f_sm2 = pl.f_sm2;
    da.f_sm2.slab = L.slabA;
  } else {
    CTN_HIP(launch_stats_finalize(L.slabA, pl.G, pl.partsA, pl.cnt, 1, 0.f, L.sums2, s));
  }
  {
    TimedScope ts(CTN_TIMER_DW_BWD, s);
    CTN_HIP(launch_dw_bwd(dt, da, s));
  }
  GemmCols c1 = pl.c1;   // (f) dW1 = gh1^T . x, gh1 = G1
  c1.A = L.G1; c1.B = x; c1.Cpart = L.cpart1; c1.nchunks = pl.chunks1;
  if (pl.fused1) {
    // (d+e) gx = n1bwd(G2) . W1 + gy; the operand stage applies the norm-1/PReLU-1
    //       backward (norm-1 sums folded from dw_bwd's slab), sums the alpha-1
    //       gradient and stores gh1 = dL/dh1 to G1 on the way (one pass instead of
    //       norm1_bwd's write + the GEMM's re-read)
    GemmRows gb = pl.gbF;
    gb.A = L.G2; gb.W = w.w1; gb.Wf = w.w1f; gb.R = gy; gb.C = gx;
    gb.aop.stats = st1; gb.aop.alpha = p->alpha1; gb.aop.aux = sv->h1; gb.aop.apart = L.alphaSlab;
    gb.aop.aout = L.G1;
    if (pl.foldX) {
      gb.aop.fold = StatFold{L.slabD, pl.partsD, pl.cnt, 0.f, 1, nullptr};
    } else {
      if (pl.fold) CTN_HIP(launch_stats_finalize(L.slabD, pl.G, pl.partsD, pl.cnt, 1, 0.f, L.sums1, s));
      gb.aop.sums = L.sums1;
    }
    {
      TimedScope ts(CTN_TIMER_GEMM_GX, s);
      CTN_HIP(launch_gemm_rows(dt, gb, s));
    }
    // everything below only produces parameter gradients: fork to sw
    if (sw != s) CTN_HIP(fork_stream(s, sw));
    {
      TimedScope ts(CTN_TIMER_COLS_W1, sw);
      CTN_HIP(launch_gemm_cols(dt, c1, sw));
    }
  } else {
    // (d) norm1 backward finish + PReLU1 backward -> G1 = dL/dh1
    DwArgs de = da;
    de.ga2 = L.G2; de.sm1 = L.sums1; de.gh1_out = L.G1; de.alpha_slab = L.alphaSlab;
    de.f_sm2 = StatFold{};
    if (pl.fold) de.f_sm1 = StatFold{L.slabD, pl.partsD, pl.cnt, 0.f, 1, nullptr};
    CTN_HIP(launch_norm1_bwd(dt, de, s));
    // (e) gx = gh1 . W1 + gy
    // (f) dW1 = gh1^T . x
    GemmRows gb = pl.gbP;
    gb.A = L.G1; gb.W = w.w1; gb.Wf = w.w1f; gb.R = gy; gb.C = gx;
    CTN_HIP(launch_gemm_rows(dt, gb, s));
    CTN_HIP(launch_gemm_cols(dt, c1, s));
    if (sw != s) CTN_HIP(fork_stream(s, sw));
  }
  // (g) all parameter-gradient partial sums
  if (defer) return CTN_OK;
  SlabBatch sb{};
  sb.nd = tb_grad_slabs(pl, L, gr, sb.d);
  CTN_HIP(launch_slab_reduce(sb, L.srtmp, sw));
  return CTN_OK;
}

extern "C" int ctn_tblock_backward(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                                   const ctn_tblock_saved* sv, const void* gy, void* gx, const ctn_tblock_grads* gr,
                                   void* ws, size_t ws_bytes, void* stream) {
  return tb_backward(d, p, x, sv, gy, gx, gr, ws, ws_bytes, (hipStream_t)stream, (hipStream_t)stream);
}

extern "C" int ctn_tblock_backward_split(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                                         const ctn_tblock_saved* sv, const void* gy, void* gx,
                                         const ctn_tblock_grads* gr, void* ws, size_t ws_bytes, void* stream,
                                         void* wgrad_stream) {
  return tb_backward(d, p, x, sv, gy, gx, gr, ws, ws_bytes, (hipStream_t)stream,
                     wgrad_stream ? (hipStream_t)wgrad_stream : (hipStream_t)stream);
}

// Which kernel each step of the block would launch: the plan's decisions, and for the
// choices the launchers make themselves, their eligibility on the plan's descriptors
extern "C" int ctn_tblock_plan(const ctn_tblock_desc* d, int backward, char* out, size_t cap) {
  int rc = tb_check(d);
  if (rc) return rc;
  if (!out || cap < 1) return fail(CTN_ERR_ARG, "null output");
  std::string s;
  if (d->norm_type == CTN_NORM_BN) {
    s = backward ? "bn:rows+cols" : "bn:rows";
  } else if (!backward) {
    const TbPlan pl = tb_plan(d, false);
    s = std::string("gemm1=") + pl.rows_kernel(pl.g1) + ",dw_fwd=" + pl.dw_kernel(false) +
        ",gemm2=" + pl.rows_kernel(pl.g2);
  } else {
    const TbPlan pl = tb_plan(d, true);
    s = std::string("pairA=") + (pl.dualA ? "dual_ws" : pl.rows_kernel(pl.ga)) + (pl.dualA ? "" : "+cols") +
        ",dw_bwd=" + pl.dw_kernel(true);
    if (pl.fused1)
      s += ",gx=ws_n1bwd,dW1=cols";
    else
      s += ",n1bwd=ew,gx+dW1=rows+cols";
  }
  if (s.size() + 1 > cap) return fail(CTN_ERR_ARG, "plan needs %zu bytes", s.size() + 1);
  memcpy(out, s.c_str(), s.size() + 1);
  return CTN_OK;
}

extern "C" size_t ctn_tblock_partials_bytes(const ctn_tblock_desc* d) {
  if (tb_check(d) != CTN_OK || d->norm_type == CTN_NORM_BN) return 0;
  return tb_layout(tb_plan(d, true), 1, nullptr, nullptr, true).part_bytes;
}

extern "C" size_t ctn_tblock_deferred_workspace_bytes(const ctn_tblock_desc* d) {
  if (tb_check(d) != CTN_OK || d->norm_type == CTN_NORM_BN) return 0;
  return tb_layout(tb_plan(d, true), 1, nullptr, nullptr, true).bytes;
}

extern "C" int ctn_tblock_backward_deferred(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                                            const ctn_tblock_saved* sv, const void* gy, void* gx,
                                            const ctn_tblock_grads* gr, void* ws, size_t ws_bytes, void* part,
                                            size_t part_bytes, void* stream) {
  return tb_backward(d, p, x, sv, gy, gx, gr, ws, ws_bytes, (hipStream_t)stream, (hipStream_t)stream, part,
                     part_bytes, true);
}

extern "C" int ctn_tblock_reduce_grads(const ctn_tblock_desc* descs, const ctn_tblock_grads* grads,
                                       void* const* parts, int n, void* stream) {
  if (n < 0 || (n > 0 && (!descs || !grads || !parts))) return fail(CTN_ERR_ARG, "null pointer");
  // an error a kernel of an earlier pass reported (device error word, copied asynchronously)
  if (int rc = dev_err_check_async()) return rc;
  std::vector<SlabDesc> sd;
  std::vector<float*> tmp;
  sd.reserve((size_t)n * 9);
  tmp.reserve((size_t)n * 9);
  for (int i = 0; i < n; ++i) {
    const ctn_tblock_desc* d = descs + i;
    int rc = tb_check(d);
    if (rc) return rc;
    if (d->norm_type == CTN_NORM_BN) return fail(CTN_ERR_UNSUPPORTED, "deferred gradient reductions: gLN / cLN only");
    if (!parts[i]) return fail(CTN_ERR_ARG, "null partials buffer (block %d)", i);
    const TbPlan pl = tb_plan(d, true);
    const TbLayout L = tb_layout(pl, 1, nullptr, parts[i], true);
    SlabDesc b[12];
    const int nb = tb_grad_slabs(pl, L, grads + i, b);
    float* t[12];
    slab_reduce_assign_tmp(b, nb, L.srtmp, t);
    for (int k = 0; k < nb; ++k) {
      sd.push_back(b[k]);
      tmp.push_back(t[k]);
    }
  }
  CTN_HIP(launch_slab_reduce_list(sd.data(), tmp.data(), (int)sd.size(), (hipStream_t)stream));
  CTN_HIP(dev_err_refresh((hipStream_t)stream));   // checked by the next pass (or ctn_device_status)
  return CTN_OK;
}
