// Comb geometry, cLN row parking and the backward tail of the depthwise kernels, shared by
// the generic lane-group kernels (ctn_tcn.hip) and the wave-item kernels (ctn_dw_wave.hip).
#pragma once
#include "ctn_common.h"
#include "ctn_kernels.h"

namespace ctn {

// ---------------------------------------------------------------------------
// Comb decomposition of the dilated depthwise conv.  Rows of one utterance are
// split into residue classes rho mod d; a work item walks rows rho + j*d for
// j in one segment of a.seg steps (dw_seg).  A lane group of H/8 lanes owns one item and
// all H channels of its rows (8 per lane, 16-byte vectors); the P taps of a
// row are consecutive comb steps, so they live in a sliding register window:
// every row is loaded and transformed once (plus P-1 halo rows per segment)
// and the next row is prefetched while the current one is computed.
// ---------------------------------------------------------------------------
struct CombGeom {
  int cg, ipw, jmax, nseg, items, wgpu;
};
__host__ __device__ inline CombGeom comb_geom(const DwArgs& a) {
  CombGeom g;
  g.cg = a.H / 8;
  g.ipw = 4 * (64 / g.cg);
  g.jmax = (a.g.Kp + a.dil - 1) / a.dil;
  g.nseg = (g.jmax + a.seg - 1) / a.seg;
  g.items = a.dil * g.nseg;
  g.wgpu = (g.items + g.ipw - 1) / g.ipw;
  return g;
}
// item id of an utterance -> residue class rho and steps [j0, j1) (empty past the last item)
CTN_DEV void comb_segment(const DwArgs& a, const CombGeom& gm, int id, int& rho, int& j0, int& j1) {
  const bool active = id < gm.items;
  rho = active ? id / gm.nseg : 0;
  j0 = active ? (id % gm.nseg) * a.seg : 0;
  j1 = active ? min(j0 + a.seg, gm.jmax) : j0;
}

// The tap that reads the output row itself, pad / dil: P-1 (causal: left pad only) or
// (P-1)/2 (centred); -1 for any other padding.
inline int dw_pown(const DwArgs& a) {
  const int pown = a.pad / a.dil;
  return pown * a.dil == a.pad && (pown == a.P - 1 || pown == (a.P - 1) / 2) ? pown : -1;
}
// the causal kernel form (for P = 1 both paddings are the centred form)
inline bool dw_causal(int pown, int P) { return pown == P - 1 && P > 1 && P - 1 != (P - 1) / 2; }

// cLN per-row sums of a comb walk.  With H = 512 one wave owns one comb item (its 64
// lanes hold all channels of each row), so a row's sums are reduced with DPP (no LDS
// round trips), parked one row per lane, and every 64 rows each lane finishes the row
// it holds: the fp64 finishing arithmetic runs once per 64 rows, not once per row.
// Narrower H (several items per wave) reduces per row over the lane group as before.
struct RowPark {
  float s = 0.f, ss = 0.f;
  int j0;   // comb step held by lane 0
  // the wave-uniform sums of step j into lane j - j0
  CTN_DEV void put(int lane, int j, float rs, float rss) {
    const int pq = j - j0;
    s = lane == pq ? rs : s;
    ss = lane == pq ? rss : ss;
  }
  // lanes < n: the finished pair (fin) or the slab entry of the row they hold, row
  // rho + (j0 + lane) * dil of the utterance at `base` (row_stat_store)
  CTN_DEV void flush(int n, int lane, int rho, int dil, int Kp, int base, int mode, int H, float eps, float2* fin,
                     double2* slab) const {
    const int k = rho + (j0 + lane) * dil;
    if (lane < n && k < Kp) row_stat_store(mode, s, ss, H, eps, fin, slab, base + k);
  }
};

// column-partial reduction: sum val[8] over the lanes that own channel group c, write H floats
CTN_DEV void col_reduce8(float* buf, const float v[8], int rl, int c, int nrl, int cg, bool act, float* dst) {
  const int H = cg * 8;
  if (act)
#pragma unroll
    for (int e = 0; e < 8; ++e) buf[rl * H + c * 8 + e] = v[e];
  __syncthreads();
  for (int ch = threadIdx.x; ch < H; ch += blockDim.x) {
    float s = 0.f;
    for (int q = 0; q < nrl; ++q) s += buf[q * H + ch];
    dst[ch] = s;
  }
  __syncthreads();
}

// Workgroup reductions after a backward walk: the column partials of gamma1, beta1,
// gamma2, beta2 and the depthwise weight into the workgroup's col_slab part (the layout of
// dw_col_off_*), alpha2, and for gLN (gln_part >= 0) the norm-1 backward sums into
// slab1[gln_part].  Thread (rl, c) of nrl x cg holds the 8 channels of group c; H = 8 cg is
// passed beside cg (a constant in the wave-item kernels, a.H in the lane-group ones: derived
// here it cost those an SGPR); buf: 256*8 floats, red: 16 doubles.  The order of LDS writes,
// barriers and sums is the summation order.
template <int P>
CTN_DEV void dw_bwd_tail(const DwArgs& a, float* buf, double* red, const float (&cgam)[8], const float (&cbet)[8],
                         const float (&cgam2)[8], const float (&cbet2)[8], const float (&cwd)[P][8], float calpha,
                         float ts, float tss, int rl, int c, int nrl, int cg, int H, long gln_part) {
  float* cs = a.col_slab + (size_t)blockIdx.x * dw_col_stride(a);
  col_reduce8(buf, cgam, rl, c, nrl, cg, true, cs + dw_col_off_gamma1(P, H));
  col_reduce8(buf, cbet, rl, c, nrl, cg, true, cs + dw_col_off_beta1(P, H));
  col_reduce8(buf, cgam2, rl, c, nrl, cg, true, cs + dw_col_off_gamma2(P, H));
  col_reduce8(buf, cbet2, rl, c, nrl, cg, true, cs + dw_col_off_beta2(P, H));
#pragma unroll
  for (int p = 0; p < P; ++p) {   // stored [H][P] to match the parameter layout [H,1,P]
#pragma unroll
    for (int e = 0; e < 8; ++e) buf[rl * H + c * 8 + e] = cwd[p][e];
    __syncthreads();
    for (int chn = threadIdx.x; chn < H; chn += blockDim.x) {
      float sacc = 0.f;
      for (int q = 0; q < nrl; ++q) sacc += buf[q * H + chn];
      cs[dw_col_off_wd(P, H) + chn * P + p] = sacc;
    }
    __syncthreads();
  }
  double v3[3] = {(double)calpha, (double)ts, (double)tss};
  block_sum_d<3>(v3, red);
  if (threadIdx.x == 0) {
    cs[dw_col_off_alpha2(P, H)] = (float)v3[0];
    if (gln_part >= 0) a.slab1[gln_part] = make_double2(v3[1], v3[2]);
  }
}

}  // namespace ctn
