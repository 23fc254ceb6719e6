// Mixture-consistency projection (Wisdom et al. 2019) on the model's outputs (gfx950); a
// sibling of ctn_mixit.hip and ctn_pit.hip.  Definition: include/ctn.h, DESIGN.md §28.
//
//   y_c[t] = s_c[t] + w_c r[t],  r[t] = x[t] - sum_j s_j[t]   (t < n; y = s beyond)
//
// mixcon_pow   : power mode.  Per utterance and T-chunk (the chunk rule of pit_stats), fp64
//                partial sums p_c = sum_{t<n} s_c[t]^2; block_sum_d's fixed order, no atomics.
// mixcon_fold_w: one workgroup per utterance.  Thread c folds the chunks of p_c in chunk
//                order; thread 0 adds P in ascending c and writes coef = {w_c, D}.
// mixcon_fwd   : element-wise, fp64 per sample, rounded to fp32 once.
// mixcon_bstat : power mode, backward.  a_c = sum_{t<n} g_c[t] r[t] per chunk, as mixcon_pow.
// mixcon_fold_k: folds a_c and writes k_c = 2 (a_c - sum_j w_j a_j) / D.
// mixcon_bwd   : element-wise.  dL/ds_k[t] = g_k[t] - G[t] + s_k[t] k_k, G = sum_c w_c g_c[t];
//                dL/dx[t] = G[t] when asked for; fp64 per sample, rounded once.
//
// Every element-wise workgroup belongs to one utterance, so n, w_c and k_c are uniform
// loads.  Loads and stores are single floats: rows start at m*C*T + c*T, which an odd T
// leaves without 16-byte (or 8-byte) alignment, and a wave's 64 consecutive floats already
// fill whole cache lines.  The per-thread state is C fp64 accumulators (statistics) or C
// samples plus C coefficients (element-wise): 32 VGPRs at C = 16, no scratch.
#include "ctn_common.h"
#include "ctn_mixcon.h"

namespace ctn {

constexpr double MIXCON_EPS = 1e-8;
constexpr int MIXCON_EW_BLOCKS = 256;   // at most this many element-wise workgroups per utterance

CTN_DEV int mixcon_len(const int64_t* lengths, int m, int T) {
  if (!lengths) return T;
  const long l = lengths[m];
  return l < 0 ? 0 : (l > T ? T : (int)l);
}

// [t0, t1) of chunk `chunk`, cut at the utterance's length
CTN_DEV void mixcon_span(const MixconArgs& a, int chunk, int n, int& t0, int& t1) {
  const int span = (a.T + a.chunks - 1) / a.chunks;
  t0 = chunk * span;
  t1 = t0 + span < a.T ? t0 + span : a.T;
  if (t1 > n) t1 = n;
}

template <int C>
__global__ __launch_bounds__(256) void mixcon_pow_kernel(MixconArgs a) {
  __shared__ double red[C * 4];
  const int m = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
  int t0, t1;
  mixcon_span(a, chunk, mixcon_len(a.lengths, m, a.T), t0, t1);
  const float* sm = a.s + (size_t)m * C * a.T;
  double p[C];
#pragma unroll
  for (int c = 0; c < C; ++c) p[c] = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += 256) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double v = (double)sm[(size_t)c * a.T + t];
      p[c] += v * v;
    }
  }
  block_sum_d<C>(p, red);
  if (threadIdx.x == 0) {
    double* o = a.slab + (size_t)blockIdx.x * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = p[c];
  }
}

template <int C>
__global__ __launch_bounds__(256) void mixcon_bstat_kernel(MixconArgs a) {
  __shared__ double red[C * 4];
  const int m = blockIdx.x / a.chunks, chunk = blockIdx.x % a.chunks;
  int t0, t1;
  mixcon_span(a, chunk, mixcon_len(a.lengths, m, a.T), t0, t1);
  const float* sm = a.s + (size_t)m * C * a.T;
  const float* gm = a.g + (size_t)m * C * a.T;
  const float* xm = a.x + (size_t)m * a.T;
  double acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0;
  for (int t = t0 + threadIdx.x; t < t1; t += 256) {
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) sum += (double)sm[(size_t)c * a.T + t];
    const double r = (double)xm[t] - sum;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] += (double)gm[(size_t)c * a.T + t] * r;
  }
  block_sum_d<C>(acc, red);
  if (threadIdx.x == 0) {
    double* o = a.slab + (size_t)blockIdx.x * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = acc[c];
  }
}

// chunk partials of value c in chunk order
CTN_DEV double mixcon_fold(const MixconArgs& a, int m, int c) {
  double v = 0.0;
  for (int ch = 0; ch < a.chunks; ++ch) v += a.slab[((size_t)m * a.chunks + ch) * a.C + c];
  return v;
}

__global__ __launch_bounds__(64) void mixcon_fold_w_kernel(MixconArgs a) {
  __shared__ double p[MIXCON_CMAX];
  const int m = blockIdx.x, C = a.C;
  if ((int)threadIdx.x < C) p[threadIdx.x] = mixcon_fold(a, m, threadIdx.x);
  __syncthreads();
  if (threadIdx.x == 0) {
    double P = 0.0;
    for (int c = 0; c < C; ++c) P += p[c];
    const double D = P + C * MIXCON_EPS;
    double* o = a.coef + (size_t)m * (C + 1);
    for (int c = 0; c < C; ++c) o[c] = (p[c] + MIXCON_EPS) / D;
    o[C] = D;
  }
}

__global__ __launch_bounds__(64) void mixcon_fold_k_kernel(MixconArgs a) {
  __shared__ double ac[MIXCON_CMAX];
  const int m = blockIdx.x, C = a.C;
  if ((int)threadIdx.x < C) ac[threadIdx.x] = mixcon_fold(a, m, threadIdx.x);
  __syncthreads();
  if (threadIdx.x == 0) {
    const double* w = a.coef + (size_t)m * (C + 1);
    double A = 0.0;
    for (int c = 0; c < C; ++c) A += w[c] * ac[c];
    for (int c = 0; c < C; ++c) a.kcoef[(size_t)m * C + c] = 2.0 * (ac[c] - A) / w[C];
  }
}

template <int C>
__global__ __launch_bounds__(256) void mixcon_fwd_kernel(MixconArgs a, int bpu) {
  const int m = blockIdx.x / bpu, j = blockIdx.x % bpu;
  const int T = a.T, n = mixcon_len(a.lengths, m, T);
  const float* sm = a.s + (size_t)m * C * T;
  const float* xm = a.x + (size_t)m * T;
  float* ym = a.y + (size_t)m * C * T;
  double w[C];
#pragma unroll
  for (int c = 0; c < C; ++c) w[c] = a.mode == MIXCON_POWER ? a.coef[(size_t)m * (C + 1) + c] : 1.0 / C;
  for (int t = j * 256 + threadIdx.x; t < T; t += bpu * 256) {
    float e[C];
#pragma unroll
    for (int c = 0; c < C; ++c) e[c] = sm[(size_t)c * T + t];
    if (t < n) {
      double sum = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) sum += (double)e[c];
      const double r = (double)xm[t] - sum;
#pragma unroll
      for (int c = 0; c < C; ++c) e[c] = (float)((double)e[c] + w[c] * r);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) ym[(size_t)c * T + t] = e[c];
  }
}

template <int C>
__global__ __launch_bounds__(256) void mixcon_bwd_kernel(MixconArgs a, int bpu) {
  const int m = blockIdx.x / bpu, j = blockIdx.x % bpu;
  const int T = a.T, n = mixcon_len(a.lengths, m, T);
  const bool power = a.mode == MIXCON_POWER;
  const float* sm = a.s + (size_t)m * C * T;
  const float* gm = a.g + (size_t)m * C * T;
  float* om = a.gs + (size_t)m * C * T;
  float* gxm = a.gx ? a.gx + (size_t)m * T : nullptr;
  double w[C], k[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    w[c] = power ? a.coef[(size_t)m * (C + 1) + c] : 1.0 / C;
    k[c] = power ? a.kcoef[(size_t)m * C + c] : 0.0;
  }
  for (int t = j * 256 + threadIdx.x; t < T; t += bpu * 256) {
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = gm[(size_t)c * T + t];
    float gx = 0.f;
    if (t < n) {
      double G = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) G += w[c] * (double)g[c];
      gx = (float)G;
      if (power) {
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = (float)((double)g[c] - G + (double)sm[(size_t)c * T + t] * k[c]);
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = (float)((double)g[c] - G);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) om[(size_t)c * T + t] = g[c];
    if (gxm) gxm[t] = gx;
  }
}

static int mixcon_bpu(const MixconArgs& a) {
  const int b = (a.T + 255) / 256;
  return b > MIXCON_EW_BLOCKS ? MIXCON_EW_BLOCKS : b;
}

template <int C>
static hipError_t mixcon_fwd_c(const MixconArgs& a, hipStream_t s) {
  if (a.mode == MIXCON_POWER) {
    hipLaunchKernelGGL(mixcon_pow_kernel<C>, dim3(a.M * a.chunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(mixcon_fold_w_kernel, dim3(a.M), dim3(64), 0, s, a);
  }
  const int bpu = mixcon_bpu(a);
  hipLaunchKernelGGL(mixcon_fwd_kernel<C>, dim3(a.M * bpu), dim3(256), 0, s, a, bpu);
  return hipGetLastError();
}

template <int C>
static hipError_t mixcon_bwd_c(const MixconArgs& a, hipStream_t s) {
  if (a.mode == MIXCON_POWER) {
    hipLaunchKernelGGL(mixcon_bstat_kernel<C>, dim3(a.M * a.chunks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(mixcon_fold_k_kernel, dim3(a.M), dim3(64), 0, s, a);
  }
  const int bpu = mixcon_bpu(a);
  hipLaunchKernelGGL(mixcon_bwd_kernel<C>, dim3(a.M * bpu), dim3(256), 0, s, a, bpu);
  return hipGetLastError();
}

#define MIXCON_DISPATCH(fn)                                                                  \
  switch (a.C) {                                                                             \
    case 2: return fn<2>(a, s);   case 3: return fn<3>(a, s);   case 4: return fn<4>(a, s);   \
    case 5: return fn<5>(a, s);   case 6: return fn<6>(a, s);   case 7: return fn<7>(a, s);   \
    case 8: return fn<8>(a, s);   case 9: return fn<9>(a, s);   case 10: return fn<10>(a, s); \
    case 11: return fn<11>(a, s); case 12: return fn<12>(a, s); case 13: return fn<13>(a, s); \
    case 14: return fn<14>(a, s); case 15: return fn<15>(a, s); case 16: return fn<16>(a, s); \
  }                                                                                          \
  return hipErrorInvalidValue

hipError_t launch_mixcon_forward(const MixconArgs& a, hipStream_t s) { MIXCON_DISPATCH(mixcon_fwd_c); }

hipError_t launch_mixcon_backward(const MixconArgs& a, hipStream_t s) { MIXCON_DISPATCH(mixcon_bwd_c); }

}  // namespace ctn
