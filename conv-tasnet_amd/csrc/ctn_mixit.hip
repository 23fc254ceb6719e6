// MixIT loss (mixture-invariant training, Wisdom et al. 2020) as batched reductions
// (gfx950); a sibling of ctn_pit.hip with the same shape: one fp64 statistics pass, a
// small search, element-wise passes.  Definition: include/ctn.h, DESIGN.md §27.
//
// mixit_stats : per utterance and T-chunk (the chunk rule of pit_stats), fp64 partial sums
//               over t < length of the C outputs, the 2 recordings, the upper triangle of
//               the outputs' Gram matrix, the C x 2 cross products and the 2 recording
//               energies: NV = C + 2 + C(C+1)/2 + 2C + 2 values (64 at C = 8).  Reads est
//               and mixtures once; block_sum_d's fixed order, no atomics.
// mixit_search: one workgroup per utterance.  Folds the chunks in chunk order, thread p
//               scores assignment p (bit c of p = recording of output c) from the
//               statistics alone in fp64, thread 0 keeps the first maximum in ascending
//               p, threads 0 and 1 write the winner's gradient coefficients.
// mixit_loss  : loss = -mean of the fp64 maxima, one fixed order.
// mixit_remix : remix[m][n][t] = sum of the outputs assigned to recording n, fp32,
//               ascending c; zero at t >= length.
// mixit_bwd   : dL/dest[m][c][t] = scale_m (al_n x_n[t] + be_n y_n[t] + off_n), n = bit c
//               of assign[m], y_n recomputed from the C outputs and the sum evaluated in
//               fp64 from the fp32 coefficients, rounded once; 0 at t >= length.
//
// The statistics stay in registers for every C <= 8: 64 fp64 accumulators are 128 VGPRs of
// the 512 a 256-thread workgroup's waves may use (pit_stats_kernel<8> holds 104 the same
// way), so nothing is staged through LDS.
#include "ctn_common.h"
#include "ctn_mixit.h"

namespace ctn {

constexpr double MIXIT_EPS = 1e-8;

int mixit_nv(int C) { return C + 2 + C * (C + 1) / 2 + 2 * C + 2; }

// statistics layout: SE[c] | SX[n] | G[j][k], j <= k, row-major | ES[c][n] | XX[n]
CTN_DEV int mixit_off_sx(int C) { return C; }
CTN_DEV int mixit_off_g(int C) { return C + 2; }
CTN_DEV int mixit_off_es(int C) { return C + 2 + C * (C + 1) / 2; }
CTN_DEV int mixit_off_xx(int C) { return C + 2 + C * (C + 1) / 2 + 2 * C; }
CTN_DEV int mixit_g_idx(int C, int j, int k) { return j * C - j * (j - 1) / 2 + (k - j); }

CTN_DEV long mixit_len(const int64_t* lengths, int m, int T) {
  const long l = lengths[m];
  return l < 0 ? 0 : (l > T ? T : l);
}

template <int C>
__global__ __launch_bounds__(256) void mixit_stats_kernel(MixitArgs a) {
  constexpr int NG = C * (C + 1) / 2, NV = C + 2 + NG + 2 * C + 2;
  constexpr int oSX = C, oG = C + 2, oES = C + 2 + NG, oXX = C + 2 + NG + 2 * C;
  __shared__ double red[NV * 4];
  const int m = blockIdx.y, chunk = blockIdx.x;
  const int T = a.T;
  const long len = mixit_len(a.lengths, m, T);
  const int span = (T + a.chunks - 1) / a.chunks;
  const int t0 = chunk * span;
  int t1 = t0 + span < T ? t0 + span : T;
  if (t1 > len) t1 = (int)len;                       // sums run over t < length only
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  const float* em = a.est + (size_t)m * C * T;
  const float* xm = a.mix + (size_t)m * 2 * T;
  for (int t = t0 + threadIdx.x; t < t1; t += 256) {
    double e[C], x[2];
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = (double)em[(size_t)c * T + t];
    x[0] = (double)xm[t];
    x[1] = (double)xm[(size_t)T + t];
    v[oSX] += x[0];
    v[oSX + 1] += x[1];
    v[oXX] += x[0] * x[0];
    v[oXX + 1] += x[1] * x[1];
    int g = oG;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      v[j] += e[j];
      v[oES + 2 * j] += e[j] * x[0];
      v[oES + 2 * j + 1] += e[j] * x[1];
#pragma unroll
      for (int k = j; k < C; ++k) v[g++] += e[j] * e[k];
    }
  }
  block_sum_d<NV>(v, red);
  if (threadIdx.x == 0) {
    double* o = a.slab + ((size_t)m * a.chunks + chunk) * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] = v[i];
  }
}

// SNR of recording n against the sum of the outputs in set S (bit c set: output c is a
// member), from the folded statistics v alone; cf (nullable) receives al, be, off of
// d score / d y_n[t] = al x_n[t] + be y_n[t] + off, score = (snr_0 + snr_1) / 2
CTN_DEV double mixit_side(const double* v, int C, unsigned S, int n, int mode, double tau, double len, double* cf) {
  double sy = 0.0, yx = 0.0, yy = 0.0;
  const double* G = v + mixit_off_g(C);
  const double* ES = v + mixit_off_es(C);
  for (int j = 0; j < C; ++j) {
    if (!((S >> j) & 1u)) continue;
    sy += v[j];
    yx += ES[2 * j + n];
    yy += G[mixit_g_idx(C, j, j)];
    double cross = 0.0;
    for (int k = j + 1; k < C; ++k)
      if ((S >> k) & 1u) cross += G[mixit_g_idx(C, j, k)];
    yy += 2.0 * cross;
  }
  const double sx = v[mixit_off_sx(C) + n], xx = v[mixit_off_xx(C) + n];
  if (mode == 0) {
    const double R = xx - 2.0 * yx + yy;
    const double den = R + tau * xx + MIXIT_EPS;
    if (cf) {
      const double k = 10.0 / (log(10.0) * den);     // 1/2 (mean of two) x 2 (d R / d y)
      cf[0] = k;
      cf[1] = -k;
      cf[2] = 0.0;
    }
    return 10.0 * log10((xx + MIXIT_EPS) / den);
  }
  // SI-SNR, pit_final_kernel's formulas on (y_n, x_n), both means over t < length
  const double eb = sy / len;
  const double Ee = yy - eb * sy;
  const double Et = xx - sx * sx / len;
  const double D = yx - eb * sx;
  const double E = Et + MIXIT_EPS;
  const double Pp = D * D * Et / (E * E);
  const double Ne = Ee - 2.0 * D * D / E + D * D * Et / (E * E);
  const double Nd = Ne + MIXIT_EPS;
  const double ratio = Pp / Nd;
  if (cf) {
    const double dsnr = 10.0 / (log(10.0) * (ratio + MIXIT_EPS));
    const double dPp = 2.0 * D * Et / (E * E);
    const double dNe = -4.0 * D / E + 2.0 * D * Et / (E * E);
    const double dr_dD = (dPp * Nd - Pp * dNe) / (Nd * Nd);
    const double dr_dEe = -Pp / (Nd * Nd);
    const double al = dsnr * dr_dD / 2.0, be = 2.0 * dsnr * dr_dEe / 2.0;
    cf[0] = al;
    cf[1] = be;
    cf[2] = -al * sx / len - be * eb;
  }
  return 10.0 * log10(ratio + MIXIT_EPS);
}

__global__ __launch_bounds__(256) void mixit_search_kernel(MixitArgs a) {
  constexpr int NVMAX = MIXIT_CMAX + 2 + MIXIT_CMAX * (MIXIT_CMAX + 1) / 2 + 2 * MIXIT_CMAX + 2;
  __shared__ double v[NVMAX], sc[256];
  __shared__ unsigned win;
  const int m = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, NV = mixit_off_xx(C) + 2;
  const unsigned np = 1u << C, full = np - 1u;
  for (int i = tid; i < NV; i += 256) {              // chunk partials in chunk order
    double s = 0.0;
    for (int ch = 0; ch < a.chunks; ++ch) s += a.slab[((size_t)m * a.chunks + ch) * NV + i];
    v[i] = s;
  }
  __syncthreads();
  const double len = (double)mixit_len(a.lengths, m, a.T);
  const unsigned p = (unsigned)tid;
  if (p < np) {
    const double s0 = mixit_side(v, C, ~p & full, 0, a.mode, a.tau, len, nullptr);
    const double s1 = mixit_side(v, C, p, 1, a.mode, a.tau, len, nullptr);
    sc[tid] = (s0 + s1) / 2.0;
  }
  __syncthreads();
  if (tid == 0) {
    double best = sc[0];
    unsigned bi = 0;
    for (unsigned q = 1; q < np; ++q)
      if (sc[q] > best || (best != best && sc[q] == sc[q])) { best = sc[q]; bi = q; }   // first maximum; a NaN never wins
    win = bi;
    a.max_snr[m] = (float)best;
    a.assign[m] = (int64_t)bi;
    a.msd[m] = best;
  }
  __syncthreads();
  if (tid < 2) {
    const unsigned S = tid == 0 ? (~win & full) : win;
    double cf[3];
    mixit_side(v, C, S, tid, a.mode, a.tau, len, cf);
    float* o = a.coef + ((size_t)m * 2 + tid) * 4;
    o[0] = (float)cf[0];
    o[1] = (float)cf[1];
    o[2] = (float)cf[2];
    o[3] = 0.f;
  }
}

// loss = -mean over utterances of max_snr: thread i takes utterances i, i + 256, ... in order
__global__ __launch_bounds__(256) void mixit_loss_kernel(MixitArgs a) {
  __shared__ double red[4];
  double l1[1] = {0.0};
  for (int m = threadIdx.x; m < a.M; m += 256) l1[0] += a.msd[m];
  block_sum_d<1>(l1, red);
  if (threadIdx.x == 0) a.loss[0] = (float)(-l1[0] / a.M);
}

// y[n] = sum of the outputs assigned to recording n, fp32, ascending c
template <int C>
CTN_DEV void mixit_sum2(const float* e, unsigned p, float* y) {
  y[0] = 0.f;
  y[1] = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const bool one = (p >> c) & 1u;
    y[0] = one ? y[0] : y[0] + e[c];
    y[1] = one ? y[1] + e[c] : y[1];
  }
}

template <int C>
__global__ __launch_bounds__(256) void mixit_remix_kernel(MixitArgs a) {
  const long total = (long)a.M * a.T;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int m = (int)(i / a.T), t = (int)(i % a.T);
    float y[2] = {0.f, 0.f};
    if (t < mixit_len(a.lengths, m, a.T)) {
      float e[C];
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = a.est[((size_t)m * C + c) * a.T + t];
      mixit_sum2<C>(e, (unsigned)a.assign[m], y);
    }
    a.remix[((size_t)m * 2) * a.T + t] = y[0];
    a.remix[((size_t)m * 2 + 1) * a.T + t] = y[1];
  }
}

template <int C>
__global__ __launch_bounds__(256) void mixit_bwd_kernel(MixitArgs a) {
  const long total = (long)a.M * a.T;
  const float gl = a.g_loss ? a.g_loss[0] : 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int m = (int)(i / a.T), t = (int)(i % a.T);
    float g[2] = {0.f, 0.f};
    const unsigned p = (unsigned)a.assign[m];
    const bool in = t < mixit_len(a.lengths, m, a.T);
    if (in) {
      // y_n and the three-term sum in fp64, rounded once: in snr mode al = -be, and near the
      // SNR ceiling x_n - y_n is ~1e-3 of x_n, which fp32 sums of y_n would leave with 1e-4
      // of relative error (the pass stays memory bound: C + 6 fp64 operations per sample)
      double y[2] = {0.0, 0.0};
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double e = (double)a.est[((size_t)m * C + c) * a.T + t];
        const bool one = (p >> c) & 1u;
        y[0] = one ? y[0] : y[0] + e;
        y[1] = one ? y[1] + e : y[1];
      }
      const float scale = (a.g_maxsnr ? a.g_maxsnr[m] : 0.f) - gl / (float)a.M;
      const float* cf = a.coef + (size_t)m * 8;
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const double x = (double)a.mix[((size_t)m * 2 + n) * a.T + t];
        g[n] = (float)((double)scale * ((double)cf[4 * n] * x + (double)cf[4 * n + 1] * y[n] + (double)cf[4 * n + 2]));
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) a.gest[((size_t)m * C + c) * a.T + t] = in ? (((p >> c) & 1u) ? g[1] : g[0]) : 0.f;
  }
}

static int mixit_ew_grid(const MixitArgs& a) {
  const long total = (long)a.M * a.T;
  const long g = (total + 255) / 256;
  return (int)(g > 4096 ? 4096 : g);
}

template <int C>
static hipError_t mixit_fwd_c(const MixitArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mixit_stats_kernel<C>, dim3(a.chunks, a.M), dim3(256), 0, s, a);
  hipLaunchKernelGGL(mixit_search_kernel, dim3(a.M), dim3(256), 0, s, a);
  hipLaunchKernelGGL(mixit_loss_kernel, dim3(1), dim3(256), 0, s, a);
  if (a.remix) hipLaunchKernelGGL(mixit_remix_kernel<C>, dim3(mixit_ew_grid(a)), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <int C>
static hipError_t mixit_bwd_c(const MixitArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(mixit_bwd_kernel<C>, dim3(mixit_ew_grid(a)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_mixit_forward(const MixitArgs& a, hipStream_t s) {
  switch (a.C) {
    case 2: return mixit_fwd_c<2>(a, s);
    case 3: return mixit_fwd_c<3>(a, s);
    case 4: return mixit_fwd_c<4>(a, s);
    case 5: return mixit_fwd_c<5>(a, s);
    case 6: return mixit_fwd_c<6>(a, s);
    case 7: return mixit_fwd_c<7>(a, s);
    case 8: return mixit_fwd_c<8>(a, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_mixit_backward(const MixitArgs& a, hipStream_t s) {
  switch (a.C) {
    case 2: return mixit_bwd_c<2>(a, s);
    case 3: return mixit_bwd_c<3>(a, s);
    case 4: return mixit_bwd_c<4>(a, s);
    case 5: return mixit_bwd_c<5>(a, s);
    case 6: return mixit_bwd_c<6>(a, s);
    case 7: return mixit_bwd_c<7>(a, s);
    case 8: return mixit_bwd_c<8>(a, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace ctn
