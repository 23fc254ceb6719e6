// Element-wise / depthwise kernels of the TemporalBlock (conv_tasnet.py:212-272), lane-group
// form, and the dispatch between them and the wave-item form (ctn_dw_wave.hip) (gfx950).
//
// dw_fwd    : n1 = norm1(PReLU(h1)) recomputed on the fly, depthwise dilated
//             conv (causal = left pad only, identical to pad + Chomp1d,
//             conv_tasnet.py:176,247-260,289), stores d (pre-PReLU) and the
//             partial statistics of PReLU(d) for norm2.
// dw_bwd    : norm2 backward (element part) -> PReLU2 backward -> transposed
//             depthwise conv -> norm1 backward partial sums; column partials
//             for gamma1/beta1/dw weight/alpha2.
// norm1_bwd : norm1 backward finish -> PReLU1 backward -> dL/dh1.
//
// Thread layout (all three): a workgroup owns 128 frame rows of one utterance
// (Kp % 128 == 0) and all H channels; a thread owns 8 consecutive channels
// (one 16-byte bf16 vector) of every (256 / (H/8))-th row.
#include "ctn_common.h"
#include "ctn_dw.h"
#include "ctn_kernels.h"

namespace ctn {

constexpr int DW_RPB = 128;   // rows per workgroup (element-wise kernels)
constexpr int DW_MAXP = 8;
constexpr int DW_MINSEG = 16; // shortest comb segment (halo rows cost (P-1)/seg)
constexpr int DW_WPS_FWD = 4, DW_WPS_BWD = 2;   // waves/SIMD the kernels' VGPR budgets allow
// comb rows prefetched per lane: 2 for bf16 (the loop is latency-bound at one row
// in flight: 8 waves x 48 B per lane per CU is half of what Little's law asks at
// 6 TB/s), 1 for fp32 (parity mode; two would exceed the VGPR budgets above)
template <typename T> constexpr int dw_pf() { return sizeof(T) == 2 ? 2 : 1; }

// Segment length such that all work items of the launch are resident at once:
// a wave owns 64/(H/8) items and walks its segment serially, so a second, partly
// filled round of waves would cost a whole segment time.  Items per utterance are
// dil * ceil(jmax/seg); when dil alone exceeds the budget the segment is the
// whole residue class (jmax steps, the shortest possible).
int dw_seg(const DwArgs& a, bool bwd) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  const long cap = (long)cus * 4 * (bwd ? DW_WPS_BWD : DW_WPS_FWD) * (64 / (a.H / 8));
  const long per_utt = cap / (a.g.M > 0 ? a.g.M : 1);
  const int jmax = (a.g.Kp + a.dil - 1) / a.dil;
  long nseg = per_utt / a.dil;
  if (nseg < 1) nseg = 1;
  int seg = (int)((jmax + nseg - 1) / nseg);
  if (seg < DW_MINSEG) seg = DW_MINSEG;
  return seg;
}
int dw_blocks(const DwArgs& a) { return a.g.M * comb_geom(a).wgpu; }
int dw_parts_per_group(const DwArgs& a) { return a.norm == NORM_GLN ? comb_geom(a).wgpu : 1; }
int ew_blocks(const DwArgs& a) { return (int)(a.g.rows() / DW_RPB); }

template <int NK> CTN_DEV float2 ld_stat(const float2* s, int m, int row) {
  return NK == NORM_GLN ? s[m] : s[row];
}

struct CombItem {
  int m, wgi, rho, j0, j1, base, c, sub;
};
// The kernels keep their per-element arithmetic in channel pairs (f32x2_t); with packed
// FP32 off (Makefile) a pair operation compiles to two scalar VALU ops.
// PReLU on a pair (an exact select, any alpha)
CTN_DEV f32x2_t pr2(f32x2_t x, float al) {
  const f32x2_t ax = x * al;
  return f32x2_t{x[0] > 0.f ? x[0] : ax[0], x[1] > 0.f ? x[1] : ax[1]};
}
CTN_DEV CombItem comb_item(const DwArgs& a, const CombGeom& gm) {
  CombItem it;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  it.c = lane % gm.cg;
  it.sub = lane / gm.cg;
  it.m = blockIdx.x / gm.wgpu;
  it.wgi = blockIdx.x % gm.wgpu;
  comb_segment(a, gm, it.wgi * gm.ipw + wv * (64 / gm.cg) + it.sub, it.rho, it.j0, it.j1);
  it.base = it.m * a.g.Kp;
  return it;
}

// ---------------------------------------------------------------------------
// dw_fwd: d[k] = sum_p w[p] n1[k - pad + p*dil],  n1 = norm1(PReLU(h1)) (0 outside [0,K))
// ---------------------------------------------------------------------------
template <typename T, int NK, int P, bool CAUSAL>
__global__ __launch_bounds__(256) void dw_fwd_kernel(DwArgs a) {
  constexpr int POWN = CAUSAL ? P - 1 : (P - 1) / 2;   // tap that reads the output row itself
  __shared__ double red[16];
  const CombGeom gm = comb_geom(a);
  const CombItem it = comb_item(a, gm);
  const int H = a.H, K = a.g.K, Kp = a.g.Kp, dil = a.dil, c = it.c;
  const T* h1 = reinterpret_cast<const T*>(a.h1);
  T* dout = reinterpret_cast<T*>(a.d_out);
  const float al1 = a.alpha1[0], al2 = a.alpha2[0];
  float2 st1u = make_float2(0.f, 0.f);
  if constexpr (NK == NORM_GLN) {
    const StatFold& f = a.f_st1;
    if (f.slab) {
      st1u = fold_stat(f, it.m);
      if (f.out && it.wgi == 0 && threadIdx.x == 0) f.out[it.m] = st1u;   // saved for backward
    } else {
      st1u = a.st1[it.m];
    }
  }

  // per-element arithmetic in channel pairs, as dw_bwd
  f32x2_t w[P][4], g1[4], b1[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ch = c * 8 + 2 * i;
    g1[i] = f32x2_t{a.gamma1[ch], a.gamma1[ch + 1]};
    b1[i] = f32x2_t{a.beta1[ch], a.beta1[ch + 1]};
#pragma unroll
    for (int p = 0; p < P; ++p) w[p][i] = f32x2_t{a.wd[ch * P + p], a.wd[(ch + 1) * P + p]};
  }
  // window win[i] = n1 at comb step j + (i - POWN), i in [0, P)
  f32x2_t win[P][4];
  auto row_of = [&](int j) { return it.rho + j * dil; };
  // cLN: the row's statistics are fetched with the row (not at the point of use,
  // where the dependent load would stall every comb step)
  auto fetch = [&](int j, Raw8<T>& r, bool& ok, int& row, float2& st) {
    const int k = row_of(j);
    ok = j >= 0 && k < K;
    row = it.base + (ok ? k : 0);
    r.load(h1 + (size_t)row * H + c * 8);
    st = NK == NORM_GLN ? st1u : a.st1[row];
  };
  auto finish = [&](const Raw8<T>& r, bool ok, float2 st, f32x2_t* out) {
    const f32x2_t nm = {-st.x, -st.x};
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // rows outside the utterance: exactly 0 (a select, so a
                                    // non-finite value in the row it fetched cannot leak in)
      const f32x2_t v = pfma((pr2(f32x2_t{r[2 * i], r[2 * i + 1]}, al1) + nm) * st.y, g1[i], b1[i]);
      out[i] = f32x2_t{ok ? v[0] : 0.f, ok ? v[1] : 0.f};
    }
  };
#pragma unroll
  for (int i = 0; i < P - 1; ++i) {           // prologue: steps j0-POWN .. j0+P-2-POWN
    Raw8<T> r; bool ok; int row; float2 st;
    fetch(it.j0 + i - POWN, r, ok, row, st);
    finish(r, ok, st, win[i]);
  }
  // DW_PF rows in flight per lane: slot q holds comb step j with j % DW_PF == q,
  // and the loop is unrolled by DW_PF so a slot is refilled (step j + DW_PF) as
  // soon as it is consumed, without register copies that would wait on a load.
  constexpr int D = dw_pf<T>();
  Raw8<T> pre[D]; bool pok[D]; int prow[D]; float2 pst[D];
#pragma unroll
  for (int q = 0; q < D; ++q) fetch(it.j0 + q + P - 1 - POWN, pre[q], pok[q], prow[q], pst[q]);
  float ts = 0.f, tss = 0.f;
  const bool wave_item = gm.cg == 64;   // one comb item per wave (see RowPark)
  const int lane = threadIdx.x & 63;
  RowPark pk;
  pk.j0 = it.j0;
  // final (mean, rstd) or the (sum, sum sq) slab entry of the rows parked in lanes < n
  auto park_flush = [&](int n) {
    pk.flush(n, lane, it.rho, dil, Kp, it.base, 0, H, a.eps, a.st2_out, a.slab2);
  };
  for (int jb = it.j0; jb < it.j1; jb += D)
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const int j = jb + q;
    if (j >= it.j1) break;
    Raw8<T> cur = pre[q]; const bool cok = pok[q]; const float2 cst = pst[q];
    if (j + D < it.j1) fetch(j + D + P - 1 - POWN, pre[q], pok[q], prow[q], pst[q]);
    finish(cur, cok, cst, win[P - 1]);
    const int k = row_of(j);
    const f32x2_t z2 = {0.f, 0.f};
    f32x2_t o2[4] = {z2, z2, z2, z2};
    float s = 0.f, ss = 0.f;
    if (k < K) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o2[i] = w[0][i] * win[0][i];
#pragma unroll
        for (int p = 1; p < P; ++p) o2[i] = pfma(w[p][i], win[p][i], o2[i]);
        const f32x2_t a2 = pr2(o2[i], al2);
        s += a2[0];   // sums over the 8 channels in channel order
        ss = fmaf(a2[0], a2[0], ss);
        s += a2[1];
        ss = fmaf(a2[1], a2[1], ss);
      }
    }
    if (k < Kp) {
      const float out[8] = {o2[0][0], o2[0][1], o2[1][0], o2[1][1], o2[2][0], o2[2][1], o2[3][0], o2[3][1]};
      Vec8<T>::store(dout + (size_t)(it.base + k) * H + c * 8, out);
    }
    if constexpr (NK == NORM_GLN) {
      ts += s;
      tss += ss;
    } else if (wave_item) {
      pk.put(lane, j, wave_sum_dpp(s), wave_sum_dpp(ss));
      if (j - pk.j0 == 63) {
        park_flush(64);
        pk.j0 = j + 1;
      }
    } else {
      s = wave_sum_group(s, gm.cg);
      ss = wave_sum_group(ss, gm.cg);
      if (c == 0 && k < Kp) row_stat_store(0, s, ss, H, a.eps, a.st2_out, a.slab2, it.base + k);
    }
#pragma unroll
    for (int i = 0; i < P - 1; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) win[i][e] = win[i + 1][e];
  }
  if constexpr (NK != NORM_GLN)
    if (wave_item && it.j1 > pk.j0) park_flush(it.j1 - pk.j0);
  if constexpr (NK == NORM_GLN) {
    double v2[2] = {(double)ts, (double)tss};
    block_sum_d<2>(v2, red);
    if (threadIdx.x == 0) a.slab2[(size_t)it.m * gm.wgpu + it.wgi] = make_double2(v2[0], v2[1]);
  }
}

// ---------------------------------------------------------------------------
// dw_bwd: dL/dd (norm2 + PReLU2 backward) on a gd window, transposed depthwise
// conv, depthwise weight gradient against an n1 window, norm1 backward sums.
//   gd window  gdw[i] = dL/dd   at step j + (POWN - P + 1 + i)
//   ah window  ahw[i] = hat a1  at step j + (i - POWN)
// ---------------------------------------------------------------------------
template <typename T, int NK, int P, bool CAUSAL>
__global__ __launch_bounds__(256) void dw_bwd_kernel(DwArgs a) {
  constexpr int POWN = CAUSAL ? P - 1 : (P - 1) / 2;
  constexpr int GT = POWN, AT = P - 1 - POWN;           // newest step of each window, relative to j
  __shared__ double red[16];
  __shared__ float buf[256 * 8];
  const CombGeom gm = comb_geom(a);
  const CombItem it = comb_item(a, gm);
  const int H = a.H, K = a.g.K, Kp = a.g.Kp, dil = a.dil, c = it.c;
  const T* h1 = reinterpret_cast<const T*>(a.h1);
  const T* dd = reinterpret_cast<const T*>(a.d);
  const T* ga2 = reinterpret_cast<const T*>(a.ga2);
  T* ga1o = reinterpret_cast<T*>(a.ga1_out);
  const float al1 = a.alpha1[0], al2 = a.alpha2[0];
  float2 st1u = make_float2(0.f, 0.f), st2u = st1u, sm2u = st1u;
  if constexpr (NK == NORM_GLN) {
    st1u = a.st1[it.m];
    st2u = a.st2[it.m];
    const StatFold& f = a.f_sm2;
    sm2u = f.slab ? fold_stat(f, it.m) : a.sm2[it.m];
  }

  // Per-element arithmetic in channel pairs (this kernel is VALU-issue-bound at 2 waves
  // per SIMD).  Pair i holds channels 2i, 2i+1 of the lane's 8.
  f32x2_t w[P][4], g1[4], b1[4], g2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ch = c * 8 + 2 * i;
    g1[i] = f32x2_t{a.gamma1[ch], a.gamma1[ch + 1]};
    b1[i] = f32x2_t{a.beta1[ch], a.beta1[ch + 1]};
    g2[i] = f32x2_t{a.gamma2[ch], a.gamma2[ch + 1]};
#pragma unroll
    for (int q = 0; q < P; ++q) w[q][i] = f32x2_t{a.wd[ch * P + q], a.wd[(ch + 1) * P + q]};
  }
  // cgam/cbet: norm-1 affine gradients; cgam2/cbet2: norm-2 affine gradients
  // (sum over own rows of g_n2 * hat a2 and of g_n2)
  f32x2_t cgam[4], cbet[4], cgam2[4], cbet2[4], cwd[P][4];
  const f32x2_t z2 = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    cgam[i] = cbet[i] = cgam2[i] = cbet2[i] = z2;
#pragma unroll
    for (int q = 0; q < P; ++q) cwd[q][i] = z2;
  }
  float calpha = 0.f, ts = 0.f, tss = 0.f;

  auto row_of = [&](int j) { return it.rho + j * dil; };
  // gd stream: d and dL/d(hat a2) of one comb step
  // (cLN statistics are loaded at the point of use here: fetching them with the rows,
  // as dw_fwd does, took this 256-VGPR kernel from 661 to 878 us at c4)
  auto fetch_g = [&](int j, Raw8<T>& rd, Raw8<T>& rg, bool& ok, int& row) {
    const int k = row_of(j);
    ok = j >= 0 && k < K;
    row = it.base + (ok ? k : 0);
    rd.load(dd + (size_t)row * H + c * 8);
    rg.load(ga2 + (size_t)row * H + c * 8);
  };
  // cLN with one comb item per wave: the per-row statistics of 64 consecutive walk steps
  // are loaded one step per lane and broadcast with v_readlane, instead of a dependent
  // global load in front of every row (bstep: the step being finished, -1 outside the walk)
  float2 bst2 = make_float2(0.f, 0.f), bsm2 = bst2, bst1 = bst2;
  int bbase = -(1 << 29), bstep = -1;
  auto bl = [&](int jj) { const int k = row_of(jj); return it.base + ((jj >= 0 && k < K) ? k : 0); };
  auto batch_load = [&](int jb) {
    bbase = jb;
    const int rgw = bl(jb + (threadIdx.x & 63) + GT), rhw = bl(jb + (threadIdx.x & 63) + AT);
    bst2 = a.st2[rgw];
    bsm2 = a.sm2[rgw];
    bst1 = a.st1[rhw];
  };
  auto bcast = [&](float2 v) { return readlane2(v, __builtin_amdgcn_readfirstlane(bstep - bbase)); };
  auto finish_g = [&](const Raw8<T>& rd, const Raw8<T>& rg, bool ok, int row, bool count, f32x2_t* gd) {
    const float2 st = NK == NORM_GLN ? st2u : (bstep >= 0 ? bcast(bst2) : a.st2[row]);
    const float2 sm = NK == NORM_GLN ? sm2u : (bstep >= 0 ? bcast(bsm2) : a.sm2[row]);
    const f32x2_t nm = {-st.x, -st.x}, nsx = {-sm.x, -sm.x}, nsy = {-sm.y, -sm.y};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2_t x = {rd[2 * i], rd[2 * i + 1]};
      const f32x2_t ah = (pr2(x, al2) + nm) * st.y;                       // hat a2
      const f32x2_t gn = {rg[2 * i], rg[2 * i + 1]};                     // dL/d(norm2 output)
      const f32x2_t ga = pfma(ah, nsy, pfma(gn, g2[i], nsx)) * st.y;     // dL/da2
      const f32x2_t dx = {x[0] > 0.f ? 1.f : al2, x[1] > 0.f ? 1.f : al2};
      const f32x2_t g = ga * dx;
      gd[i] = f32x2_t{ok ? g[0] : 0.f, ok ? g[1] : 0.f};   // rows outside the utterance: exactly 0
      if (ok && count) {
        calpha = fmaf(ga[0], x[0] > 0.f ? 0.f : x[0], calpha);   // channel order
        calpha = fmaf(ga[1], x[1] > 0.f ? 0.f : x[1], calpha);
        cgam2[i] = pfma(gn, ah, cgam2[i]);
        cbet2[i] += gn;
      }
    }
  };
  // ah stream: hat a1 of one comb step
  auto fetch_h = [&](int j, Raw8<T>& rh, bool& ok, int& row) {
    const int k = row_of(j);
    ok = j >= 0 && k < K;
    row = it.base + (ok ? k : 0);
    rh.load(h1 + (size_t)row * H + c * 8);
  };
  auto finish_h = [&](const Raw8<T>& rh, int row, f32x2_t* ah) {
    const float2 st = NK == NORM_GLN ? st1u : (bstep >= 0 ? bcast(bst1) : a.st1[row]);
    const f32x2_t nm = {-st.x, -st.x};
#pragma unroll
    for (int i = 0; i < 4; ++i) ah[i] = (pr2(f32x2_t{rh[2 * i], rh[2 * i + 1]}, al1) + nm) * st.y;
  };

  // nw: the depthwise-weight gradient's operand of each window row, n1 = gamma1 * hat a1 +
  // beta1 (0 for rows outside the utterance), formed once when the row enters the window
  // instead of at each of its P uses
  f32x2_t gdw[P][4], ahw[P][4], nw[P][4];
  auto enter_n = [&](int q, bool ok) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const f32x2_t n = pfma(ahw[q][i], g1[i], b1[i]);
      nw[q][i] = f32x2_t{ok ? n[0] : 0.f, ok ? n[1] : 0.f};
    }
  };
#pragma unroll
  for (int i = 0; i < P - 1; ++i) {
    Raw8<T> rd, rg, rh; bool ok, okh; int row, rowh;
    const int sg = it.j0 + GT - P + 1 + i;
    fetch_g(sg, rd, rg, ok, row);
    fetch_h(it.j0 + AT - P + 1 + i, rh, okh, rowh);
    finish_g(rd, rg, ok, row, sg >= it.j0 && sg < it.j1, gdw[i]);   // alpha2 term: own rows only
    finish_h(rh, rowh, ahw[i]);
    enter_n(i, okh);
  }
  constexpr int D = dw_pf<T>();   // rows in flight per lane, slots as in dw_fwd
  const bool wave_item = gm.cg == 64;   // one comb item per wave (see RowPark)
  const int lane = threadIdx.x & 63;
  RowPark pk;
  pk.j0 = it.j0;
  // final norm-1 backward means or the slab entry of the rows parked in lanes < n
  auto park_flush = [&](int n) {
    pk.flush(n, lane, it.rho, dil, Kp, it.base, 1, H, a.eps, a.sm1_out, a.slab1);
  };
  // one step of the walk: row j's operands (d, dL/dn2 of step j+GT; h1 of step j+AT)
  auto body = [&](int j, const Raw8<T>& cd, const Raw8<T>& cgv, const Raw8<T>& ch, bool cok, bool cokh, int crow,
                  int crowh) __attribute__((always_inline)) {
    finish_g(cd, cgv, cok, crow, j + GT < it.j1, gdw[P - 1]);   // halo rows are counted by their own segment
    finish_h(ch, crowh, ahw[P - 1]);
    enter_n(P - 1, cokh);
    const int k = row_of(j);
    f32x2_t ga1[4] = {z2, z2, z2, z2};
    float s = 0.f, ss = 0.f;
    if (k < K) {
      f32x2_t gn1[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        gn1[i] = w[0][i] * gdw[P - 1][i];
#pragma unroll
        for (int q = 1; q < P; ++q) gn1[i] = pfma(w[q][i], gdw[P - 1 - q][i], gn1[i]);
      }
#pragma unroll
      for (int q = 0; q < P; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) cwd[q][i] = pfma(gdw[P - 1 - POWN][i], nw[q][i], cwd[q][i]);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x2_t ah = ahw[POWN][i];
        cgam[i] = pfma(gn1[i], ah, cgam[i]);
        cbet[i] += gn1[i];
        ga1[i] = gn1[i] * g1[i];
        s += ga1[i][0];   // sums over the 8 channels in channel order
        ss = fmaf(ga1[i][0], ah[0], ss);
        s += ga1[i][1];
        ss = fmaf(ga1[i][1], ah[1], ss);
      }
    }
    if (k < Kp) {
      const float o[8] = {ga1[0][0], ga1[0][1], ga1[1][0], ga1[1][1], ga1[2][0], ga1[2][1], ga1[3][0], ga1[3][1]};
      Vec8<T>::store(ga1o + (size_t)(it.base + k) * H + c * 8, o);
    }
    if constexpr (NK == NORM_GLN) {
      ts += s;
      tss += ss;
    } else if (wave_item) {
      pk.put(lane, j, wave_sum_dpp(s), wave_sum_dpp(ss));
      if (j - pk.j0 == 63) {
        park_flush(64);
        pk.j0 = j + 1;
      }
    } else {
      s = wave_sum_group(s, gm.cg);
      ss = wave_sum_group(ss, gm.cg);
      if (c == 0 && k < Kp) row_stat_store(1, s, ss, H, a.eps, a.sm1_out, a.slab1, it.base + k);
    }
#pragma unroll
    for (int i = 0; i < P - 1; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        gdw[i][e] = gdw[i + 1][e];
        ahw[i][e] = ahw[i + 1][e];
        nw[i][e] = nw[i + 1][e];
      }
  };
  Raw8<T> pd[D], pg[D], ph[D]; bool pok[D], pokh[D]; int prow[D], prowh[D];
#pragma unroll
  for (int q = 0; q < D; ++q) {
    fetch_g(it.j0 + q + GT, pd[q], pg[q], pok[q], prow[q]);
    fetch_h(it.j0 + q + AT, ph[q], pokh[q], prowh[q]);
  }
  for (int jb = it.j0; jb < it.j1; jb += D)
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const int j = jb + q;
    if (j >= it.j1) break;
    Raw8<T> cd = pd[q], cgv = pg[q], ch = ph[q];
    const bool cok = pok[q], cokh = pokh[q];
    const int crow = prow[q], crowh = prowh[q];
    if (j + D < it.j1) {
      fetch_g(j + D + GT, pd[q], pg[q], pok[q], prow[q]);
      fetch_h(j + D + AT, ph[q], pokh[q], prowh[q]);
    }
    if constexpr (NK != NORM_GLN) {   // per-row statistics of 64 walk steps per lane, broadcast by v_readlane
      if (wave_item) {
        if (j - bbase >= 64) batch_load(j);
        bstep = j;
      }
    }
    body(j, cd, cgv, ch, cok, cokh, crow, crowh);
  }
  if constexpr (NK != NORM_GLN)
    if (wave_item && it.j1 > pk.j0) park_flush(it.j1 - pk.j0);
  // ---- workgroup reductions: column partials, alpha2, norm1 sums
  auto unpair = [](const f32x2_t (&v)[4], float (&o)[8]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { o[2 * i] = v[i][0]; o[2 * i + 1] = v[i][1]; }
  };
  float ogam[8], obet[8], ogam2[8], obet2[8], owd[P][8];
  unpair(cgam, ogam);
  unpair(cbet, obet);
  unpair(cgam2, ogam2);
  unpair(cbet2, obet2);
#pragma unroll
  for (int p = 0; p < P; ++p) unpair(cwd[p], owd[p]);
  dw_bwd_tail<P>(a, buf, red, ogam, obet, ogam2, obet2, owd, calpha, ts, tss, threadIdx.x / gm.cg, c, 256 / gm.cg,
                 gm.cg, H, NK == NORM_GLN ? (long)it.m * gm.wgpu + it.wgi : -1L);
}

// ---------------------------------------------------------------------------
template <typename T, int NK>
__global__ __launch_bounds__(256) void norm1_bwd_kernel(DwArgs a) {
  __shared__ double red[8];
  const int H = a.H, cg = H / 8;
  int nrl = 256 / cg;
  if (nrl > DW_RPB) nrl = DW_RPB;
  const int tid = threadIdx.x, c = tid % cg, rl = tid / cg;
  const bool act = rl < nrl;
  const int K = a.g.K, Kp = a.g.Kp;
  const int row0 = blockIdx.x * DW_RPB, m = row0 / Kp, base = m * Kp;
  const T* h1 = reinterpret_cast<const T*>(a.h1);
  const T* ga1 = reinterpret_cast<const T*>(a.ga2);   // input: dL/d(hat a1)
  T* gh = reinterpret_cast<T*>(a.gh1_out);
  const float al1 = a.alpha1[0];
  float calpha = 0.f;
  float2 sm1u = make_float2(0.f, 0.f);
  if constexpr (NK == NORM_GLN) {
    const StatFold& f = a.f_sm1;
    sm1u = f.slab ? fold_stat(f, m) : a.sm1[m];
  }
  if (act) {
    for (int rr = rl; rr < DW_RPB; rr += nrl) {
      const int r = row0 + rr, k = r - base;
      float out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if (k < K) {
        float v[8], g[8];
        Vec8<T>::load(h1 + (size_t)r * H + c * 8, v);
        Vec8<T>::load(ga1 + (size_t)r * H + c * 8, g);
        const float2 st = ld_stat<NK>(a.st1, m, r);
        const float2 sm = NK == NORM_GLN ? sm1u : a.sm1[r];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ah = (prelu(v[e], al1) - st.x) * st.y;
          const float ga = st.y * (g[e] - sm.x - ah * sm.y);
          out[e] = ga * prelu_dx(v[e], al1);
          calpha += ga * prelu_da(v[e]);
        }
      }
      Vec8<T>::store(gh + (size_t)r * H + c * 8, out);
    }
  }
  double v1[1] = {(double)calpha};
  block_sum_d<1>(v1, red);
  if (tid == 0) a.alpha_slab[blockIdx.x] = (float)v1[0];
}


static hipError_t dw_check(const DwArgs& a) {
  const int cg = a.H / 8;
  if (a.H % 8 != 0 || cg > 64 || (cg & (cg - 1)) || a.P < 1 || a.P > DW_MAXP || a.g.Kp % DW_RPB != 0 ||
      a.dil < 1 || a.seg < 1 || dw_pown(a) < 0)
    return hipErrorInvalidValue;
  return hipSuccess;
}

// One selection of dt x norm x P (1..8) x causal for the forward and the backward: K names
// the lane-group kernel template and the wave-item launcher.
struct DwFwd {
  template <typename T, int NK, int P, bool C> static constexpr auto kernel = dw_fwd_kernel<T, NK, P, C>;
  static constexpr auto wave = launch_dw_fwd_wave;
};
struct DwBwd {
  template <typename T, int NK, int P, bool C> static constexpr auto kernel = dw_bwd_kernel<T, NK, P, C>;
  static constexpr auto wave = launch_dw_bwd_wave;
};
template <class K, typename T, int NK, int P>
static hipError_t dw_launch(const DwArgs& a, hipStream_t s) {
  const dim3 grid(dw_blocks(a)), blk(256);
  if (dw_causal(dw_pown(a), P)) hipLaunchKernelGGL((K::template kernel<T, NK, P, true>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((K::template kernel<T, NK, P, false>), grid, blk, 0, s, a);
  return hipGetLastError();
}
template <class K, typename T, int NK, int... Ps>
static hipError_t dw_dispatch_p(const DwArgs& a, hipStream_t s, std::integer_sequence<int, Ps...>) {
  hipError_t e = hipErrorInvalidValue;   // P outside 1..DW_MAXP
  // the one Ps + 1 that equals a.P launches its instantiation
  ((a.P == Ps + 1 ? (void)(e = dw_launch<K, T, NK, Ps + 1>(a, s)) : (void)0), ...);
  return e;
}
template <class K>
static hipError_t dw_dispatch(DType dt, const DwArgs& a, hipStream_t s) {
  const hipError_t e = dw_check(a);
  if (e != hipSuccess) return e;
  if (dw_wave_eligible(dt, a)) return K::wave(a, s);
  const std::make_integer_sequence<int, DW_MAXP> ps;
  if (dt == BF16)
    return a.norm == NORM_GLN ? dw_dispatch_p<K, bf16raw, NORM_GLN>(a, s, ps) : dw_dispatch_p<K, bf16raw, NORM_CLN>(a, s, ps);
  return a.norm == NORM_GLN ? dw_dispatch_p<K, float, NORM_GLN>(a, s, ps) : dw_dispatch_p<K, float, NORM_CLN>(a, s, ps);
}
hipError_t launch_dw_fwd(DType dt, const DwArgs& a, hipStream_t s) { return dw_dispatch<DwFwd>(dt, a, s); }
hipError_t launch_dw_bwd(DType dt, const DwArgs& a, hipStream_t s) { return dw_dispatch<DwBwd>(dt, a, s); }

hipError_t launch_norm1_bwd(DType dt, const DwArgs& a, hipStream_t s) {
  hipError_t e = dw_check(a);
  if (e != hipSuccess) return e;
  const dim3 grid(ew_blocks(a)), blk(256);
  if (dt == BF16) {
    if (a.norm == NORM_GLN) hipLaunchKernelGGL((norm1_bwd_kernel<bf16raw, NORM_GLN>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((norm1_bwd_kernel<bf16raw, NORM_CLN>), grid, blk, 0, s, a);
  } else {
    if (a.norm == NORM_GLN) hipLaunchKernelGGL((norm1_bwd_kernel<float, NORM_GLN>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((norm1_bwd_kernel<float, NORM_CLN>), grid, blk, 0, s, a);
  }
  return hipGetLastError();
}

}  // namespace ctn
