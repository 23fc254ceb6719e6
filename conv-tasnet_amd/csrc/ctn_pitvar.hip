// PIT loss with silent sources (Wisdom et al. 2021, "What's all the FUSS about free universal
// sound separation data?", §4) as batched reductions (gfx950); a sibling of ctn_pit.hip and
// ctn_mixit.hip with the same shape.  Definition: include/ctn.h, DESIGN.md §29.
//
// pitvar_stats: per utterance and T-chunk (the chunk rule of pit_stats), fp64 partial sums
//               over t < length of e_i^2, s_j^2, e_i, s_j, e_i s_j and x^2, x the mixture or,
//               without one, the sum of the references in ascending j: NV = 4C + C^2 + 1
//               values (97 at C = 8).  block_sum_d's fixed order, no atomics.
// pitvar_final: one workgroup per utterance.  Folds the chunks in chunk order, thread (i, j)
//               scores output i against reference j (an active reference by SNR or SI-SNR, a
//               silent one by the output's level under the mixture's), the C! <= 40320
//               permutation ranks are split over the threads and reduced by rank (the first
//               maximum in itertools.permutations order, as pit_final_wide), and thread i
//               writes output i's reference and gradient coefficients.
// pitvar_loss : loss = -mean of the fp64 maxima, one fixed order.
// pitvar_bwd  : dL/de_i[t] = scale_m (al s_j[t] + be e_i[t] + off), j = perm[i], evaluated in
//               fp64 from the fp32 coefficients and rounded once; 0 at t >= length.
//
// The statistics stay in registers for every C <= 8: 97 fp64 accumulators are 194 VGPRs of the
// 512 a 256-thread workgroup's waves may use (pit_stats_kernel<8> holds 104 the same way).
#include "ctn_common.h"
#include "ctn_pit_perm.h"
#include "ctn_pitvar.h"

namespace ctn {

constexpr double PITVAR_EPS = 1e-8;

int pitvar_nv(int C) { return 4 * C + C * C + 1; }

// statistics layout: EE[i] | TT[j] | SE[i] | SS[j] | ES[i][j] | X
CTN_DEV long pitvar_len(const int64_t* lengths, int m, int T) {
  const long l = lengths[m];
  return l < 0 ? 0 : (l > T ? T : l);
}

template <int C, bool MIX>
__global__ __launch_bounds__(256) void pitvar_stats_kernel(PitVarArgs a) {
  constexpr int NV = 4 * C + C * C + 1;
  __shared__ double red[NV * 4];
  const int m = blockIdx.y, chunk = blockIdx.x;
  const int T = a.T;
  const long len = pitvar_len(a.lengths, m, T);
  const int span = (T + a.chunks - 1) / a.chunks;
  const int t0 = chunk * span;
  int t1 = t0 + span < T ? t0 + span : T;
  if (t1 > len) t1 = (int)len;                       // sums run over t < length only
  double v[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  const float* em = a.est + (size_t)m * C * T;
  const float* sm = a.src + (size_t)m * C * T;
  for (int t = t0 + threadIdx.x; t < t1; t += 256) {
    double e[C], s[C], x = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      e[c] = (double)em[(size_t)c * T + t];
      s[c] = (double)sm[(size_t)c * T + t];
      if constexpr (!MIX) x += s[c];
    }
    if constexpr (MIX) x = (double)a.mix[(size_t)m * T + t];
    v[4 * C + C * C] += x * x;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      v[i] += e[i] * e[i];
      v[C + i] += s[i] * s[i];
      v[2 * C + i] += e[i];
      v[3 * C + i] += s[i];
#pragma unroll
      for (int j = 0; j < C; ++j) v[4 * C + i * C + j] += e[i] * s[j];
    }
  }
  block_sum_d<NV>(v, red);
  if (threadIdx.x == 0) {
    double* o = a.slab + ((size_t)m * a.chunks + chunk) * NV;
#pragma unroll
    for (int i = 0; i < NV; ++i) o[i] = v[i];
  }
}

// score of output i against reference j from the folded statistics v alone; cf (nullable)
// receives al, be, off of d max_snr / d e_i[t] = al s_j[t] + be e_i[t] + off (max_snr = sum / C)
CTN_DEV double pitvar_pair(const double* v, int C, int i, int j, bool active, int mode, double tau, double tau0,
                           double n, double* cf) {
  const double EE = v[i], TT = v[C + j], SE = v[2 * C + i], SS = v[3 * C + j], ES = v[4 * C + i * C + j];
  if (!active) {                                     // the output's level under the mixture's
    const double X = v[4 * C + C * C];
    const double den = EE + tau0 * X + PITVAR_EPS;
    if (cf) {
      cf[0] = 0.0;
      cf[1] = -20.0 / (log(10.0) * den * C);
      cf[2] = 0.0;
    }
    return 10.0 * log10((X + PITVAR_EPS) / den);
  }
  if (mode == 0) {
    const double R = TT - 2.0 * ES + EE;             // sum (s_j - e_i)^2 from the Gram sums
    const double den = R + tau * TT + PITVAR_EPS;
    if (cf) {
      const double k = 20.0 / (log(10.0) * den * C);
      cf[0] = k;
      cf[1] = -k;
      cf[2] = 0.0;
    }
    return 10.0 * log10((TT + PITVAR_EPS) / den);
  }
  // SI-SNR, pit_final_kernel's formulas, both means over t < length
  const double eb = SE / n, sb = SS / n;
  const double Ee = EE - 2.0 * eb * SE + n * eb * eb;
  const double Et = TT - 2.0 * sb * SS + n * sb * sb;
  const double D = ES - eb * SS;                     // as pit_final: sb (SE - n eb) = 0 left out
  const double E = Et + PITVAR_EPS;
  const double Pp = D * D * Et / (E * E);
  const double Ne = Ee - 2.0 * D * D / E + D * D * Et / (E * E);
  const double Nd = Ne + PITVAR_EPS;
  const double ratio = Pp / Nd;
  if (cf) {
    const double dsnr = 10.0 / (log(10.0) * (ratio + PITVAR_EPS));
    const double dPp = 2.0 * D * Et / (E * E);
    const double dNe = -4.0 * D / E + 2.0 * D * Et / (E * E);
    const double dr_dD = (dPp * Nd - Pp * dNe) / (Nd * Nd);
    const double dr_dEe = -Pp / (Nd * Nd);
    const double al = dsnr * dr_dD / C, be = 2.0 * dsnr * dr_dEe / C;
    cf[0] = al;
    cf[1] = be;
    cf[2] = -al * SS / n - be * eb;
  }
  return 10.0 * log10(ratio + PITVAR_EPS);
}

__global__ __launch_bounds__(256) void pitvar_final_kernel(PitVarArgs a) {
  constexpr int CM = PITVAR_CMAX, NVMAX = 4 * CM + CM * CM + 1;
  __shared__ double v[NVMAX], sc[CM][CM], bv[256];
  __shared__ int bp[256], win[CM];
  __shared__ bool act[CM];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int C = a.C, NV = 4 * C + C * C + 1;
  for (int i = tid; i < NV; i += 256) {              // chunk partials in chunk order
    double s = 0.0;
    for (int ch = 0; ch < a.chunks; ++ch) s += a.slab[((size_t)m * a.chunks + ch) * NV + i];
    v[i] = s;
  }
  __syncthreads();
  const double n = (double)pitvar_len(a.lengths, m, a.T);
  if (tid < C) {
    act[tid] = v[C + tid] > 0.0;                     // a sum of squares: > 0 iff a sample is not +-0
    a.active[(size_t)m * C + tid] = act[tid] ? 1 : 0;
  }
  __syncthreads();
  if (tid < C * C) {
    const int i = tid / C, j = tid % C;
    sc[i][j] = pitvar_pair(v, C, i, j, act[j], a.mode, a.tau, a.tau0, n, nullptr);
  }
  __syncthreads();
  int nperm = 1;
  for (int i = 2; i <= C; ++i) nperm *= i;
  double best = -1e300;
  int bi = nperm;                                    // no rank yet
  for (int p = tid; p < nperm; p += 256) {
    int pm[CM];
    pit_decode(p, C, pm);
    double sv = 0.0;
    for (int i = 0; i < C; ++i) sv += sc[i][pm[i]];
    if (sv > best) { best = sv; bi = p; }            // ascending p: first maximum of this thread
  }
  bv[tid] = best;
  bp[tid] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t)                    // first maximum over all ranks
      if (bv[t] > best || (bv[t] == best && bp[t] < bi)) { best = bv[t]; bi = bp[t]; }
    int pm[CM];
    if (bi >= nperm) {                               // every sum is NaN: the identity, and its sum
      bi = 0;
      best = 0.0;
      for (int i = 0; i < C; ++i) best += sc[i][i];
    }
    pit_decode(bi, C, pm);
    for (int i = 0; i < C; ++i) win[i] = pm[i];
    const double ms = best / C;
    a.max_snr[m] = (float)ms;
    a.msd[m] = ms;
  }
  __syncthreads();
  if (tid < C) {
    const int j = win[tid];
    double cf[3];
    pitvar_pair(v, C, tid, j, act[j], a.mode, a.tau, a.tau0, n, cf);
    a.perm[(size_t)m * C + tid] = j;
    float* o = a.coef + ((size_t)m * C + tid) * 4;
    o[0] = (float)cf[0];
    o[1] = (float)cf[1];
    o[2] = (float)cf[2];
    o[3] = (float)j;
  }
}

// loss = -mean over utterances of max_snr: thread i takes utterances i, i + 256, ... in order
__global__ __launch_bounds__(256) void pitvar_loss_kernel(PitVarArgs a) {
  __shared__ double red[4];
  double l1[1] = {0.0};
  for (int m = threadIdx.x; m < a.M; m += 256) l1[0] += a.msd[m];
  block_sum_d<1>(l1, red);
  if (threadIdx.x == 0) a.loss[0] = (float)(-l1[0] / a.M);
}

__global__ __launch_bounds__(256) void pitvar_bwd_kernel(PitVarArgs a) {
  const int C = a.C;
  const long total = (long)a.M * C * a.T;
  const float gl = a.g_loss ? a.g_loss[0] : 0.f;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int t = (int)(i % a.T);
    const int mi = (int)(i / a.T), m = mi / C;
    float g = 0.f;
    if (t < pitvar_len(a.lengths, m, a.T)) {
      // in snr mode al = -be, and near the SNR ceiling s - e is ~1e-3 of s: the three-term sum
      // is formed in fp64 and rounded once (the pass stays memory bound)
      const float scale = (a.g_maxsnr ? a.g_maxsnr[m] : 0.f) - gl / (float)a.M;
      const float* cf = a.coef + (size_t)mi * 4;
      const int j = (int)cf[3];
      const double s = (double)a.src[((size_t)m * C + j) * a.T + t];
      const double e = (double)a.est[i];
      g = (float)((double)scale * ((double)cf[0] * s + (double)cf[1] * e + (double)cf[2]));
    }
    a.gest[i] = g;
  }
}

template <int C>
static hipError_t pitvar_fwd_c(const PitVarArgs& a, hipStream_t s) {
  if (a.mix) hipLaunchKernelGGL((pitvar_stats_kernel<C, true>), dim3(a.chunks, a.M), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((pitvar_stats_kernel<C, false>), dim3(a.chunks, a.M), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pitvar_final_kernel, dim3(a.M), dim3(256), 0, s, a);
  hipLaunchKernelGGL(pitvar_loss_kernel, dim3(1), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_pitvar_forward(const PitVarArgs& a, hipStream_t s) {
  switch (a.C) {
    case 2: return pitvar_fwd_c<2>(a, s);
    case 3: return pitvar_fwd_c<3>(a, s);
    case 4: return pitvar_fwd_c<4>(a, s);
    case 5: return pitvar_fwd_c<5>(a, s);
    case 6: return pitvar_fwd_c<6>(a, s);
    case 7: return pitvar_fwd_c<7>(a, s);
    case 8: return pitvar_fwd_c<8>(a, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_pitvar_backward(const PitVarArgs& a, hipStream_t s) {
  if (a.C < PITVAR_CMIN || a.C > PITVAR_CMAX) return hipErrorInvalidValue;
  const long total = (long)a.M * a.C * a.T;
  const long g = (total + 255) / 256;
  hipLaunchKernelGGL(pitvar_bwd_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace ctn
