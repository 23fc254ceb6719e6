// Windowed separation of a recording of any length (include/ctn.h ctn_stitch_*, DESIGN.md
// §23): the windows of the mixture, and the joining of the model's per-window outputs
// P [J][C][W]: per-boundary C x C correlation in fp64, permutation search, chain scan and
// the permuted cross-fade overlap-add.  No atomics: every sum has one documented order, so
// the results are the same bits on every run.
#include "ctn_stitch.h"

// The cross-fade's multiply, subtract and add stay separate operations, each rounded: plain
// operators written under this pragma (the rounding-mode intrinsics are operators compiled
// in their header, where contraction is on, and get fused).
#pragma clang fp contract(off)

namespace ctn {

// ---------------------------------------------------------------------------
// frame: win[j][w] = x[j Hs + w], zeros at and past T.  One thread per four samples.
// ---------------------------------------------------------------------------
template <bool VEC> __global__ __launch_bounds__(STITCH_THREADS) void stitch_frame_kernel(StitchArgs a) {
  const int per = (a.W + 4 * STITCH_THREADS - 1) / (4 * STITCH_THREADS);
  const int j = blockIdx.x / per;
  const int w0 = 4 * ((blockIdx.x % per) * STITCH_THREADS + (int)threadIdx.x);
  if (w0 >= a.W) return;
  const long g = (long)j * a.Hs + w0;
  float* dst = a.win + (long)j * a.W + w0;
  if constexpr (VEC) {
    float4 v;
    if (g + 3 < a.T) {
      v = *reinterpret_cast<const float4*>(a.x + g);
    } else {
      v.x = g < a.T ? a.x[g] : 0.f;
      v.y = g + 1 < a.T ? a.x[g + 1] : 0.f;
      v.z = g + 2 < a.T ? a.x[g + 2] : 0.f;
      v.w = 0.f;
    }
    *reinterpret_cast<float4*>(dst) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (w0 + e < a.W) dst[e] = g + e < a.T ? a.x[g + e] : 0.f;
  }
}

// ---------------------------------------------------------------------------
// correlation.  Workgroup (boundary j, chunk ch) covers the overlap samples
// [ch 2048, ch 2048 + 2048); thread t takes, in this order, u = ch 2048 + h 1024 + 4 t + e for
// h = 0, 1 and e = 0 ... 3 (samples at or past O add nothing) and accumulates all C^2 pairs from
// +0 in fp64: every overlap sample is loaded once, 2 C O loads per boundary.  A product of
// two fp32 values is exact in fp64, so fused and unfused accumulation round alike.  The 256
// thread sums of a pair are then added in a fixed tree: within a wave v[l] += v[l + s] for
// s = 32, 16, ..., 1, then ((w0 + w1) + w2) + w3 over the four waves.
// ---------------------------------------------------------------------------
template <int C, bool VEC> __global__ __launch_bounds__(STITCH_THREADS) void stitch_corr_kernel(StitchArgs a) {
  __shared__ double red[STITCH_THREADS / 64][C * C];
  const int nb = blockIdx.x / a.nchunk, ch = blockIdx.x % a.nchunk;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* prev = a.P + (long)nb * C * a.W + a.Hs;
  const float* cur = a.P + (long)(nb + 1) * C * a.W;
  double acc[C][C];
#pragma unroll
  for (int i = 0; i < C; ++i)
#pragma unroll
    for (int k = 0; k < C; ++k) acc[i][k] = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int u0 = ch * STITCH_CHUNK + h * (STITCH_CHUNK / 2) + 4 * tid;
    float p[C][4], q[C][4];
    if (VEC) {
      if (u0 < a.O) {   // O is a multiple of 4: the whole group is inside
#pragma unroll
        for (int i = 0; i < C; ++i) {
          const float4 vp = *reinterpret_cast<const float4*>(prev + (long)i * a.W + u0);
          const float4 vq = *reinterpret_cast<const float4*>(cur + (long)i * a.W + u0);
          p[i][0] = vp.x; p[i][1] = vp.y; p[i][2] = vp.z; p[i][3] = vp.w;
          q[i][0] = vq.x; q[i][1] = vq.y; q[i][2] = vq.z; q[i][3] = vq.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < C; ++i)
#pragma unroll
          for (int e = 0; e < 4; ++e) p[i][e] = q[i][e] = 0.f;
      }
    } else {
#pragma unroll
      for (int i = 0; i < C; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const bool in = u0 + e < a.O;
          p[i][e] = in ? prev[(long)i * a.W + u0 + e] : 0.f;
          q[i][e] = in ? cur[(long)i * a.W + u0 + e] : 0.f;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int i = 0; i < C; ++i)
#pragma unroll
        for (int k = 0; k < C; ++k) acc[i][k] = fma((double)p[i][e], (double)q[k][e], acc[i][k]);
  }
#pragma unroll
  for (int i = 0; i < C; ++i)
#pragma unroll
    for (int k = 0; k < C; ++k) {
      double v = acc[i][k];
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
      if (lane == 0) red[wid][i * C + k] = v;
    }
  __syncthreads();
  if (tid < C * C)
    a.part[((long)nb * a.nchunk + ch) * (C * C) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ---------------------------------------------------------------------------
// permutation search: one wave per window j.  j = 0 has no boundary (identity, status 0,
// S = 0).  Lanes < C^2 finish S_j from +0 over the chunks in index order.  The C!
// permutations are numbered in lexicographic (itertools.permutations) order; lane l scores
// k = l, l + 64, ... as ((S[0][pi 0] + S[1][pi 1]) + ...) and keeps a later one only on
// strictly greater; across lanes the greater score wins and, on equal scores, the lower k:
// the first maximiser.  A non-finite entry of S_j: identity, status 1.
// ---------------------------------------------------------------------------
template <int N> struct Fact { static constexpr int v = N * Fact<N - 1>::v; };
template <> struct Fact<0> { static constexpr int v = 1; };

// k-th permutation of 0 ... C-1 in lexicographic order, one nibble per position
template <int C> CTN_DEV uint32_t stitch_kth_perm(int k, const double* S, double* score) {
  uint64_t rem = 0x76543210ull;
  uint32_t pk = 0;
  double sc = 0.0;
  static_for<C>([&](auto ic) {
    constexpr int i = decltype(ic)::value;
    constexpr int f = Fact<C - 1 - i>::v;
    const int d = k / f;
    k -= d * f;
    const int sh = 4 * d;
    const int v = (int)((rem >> sh) & 15u);
    rem = (rem & ((1ull << sh) - 1ull)) | ((rem >> (sh + 4)) << sh);
    pk |= (uint32_t)v << (4 * i);
    if (S) sc = i == 0 ? S[v] : sc + S[i * C + v];
  });
  if (score) *score = sc;
  return pk;
}

template <int C> __global__ __launch_bounds__(STITCH_THREADS) void stitch_perm_kernel(StitchArgs a) {
  __shared__ double sS[STITCH_THREADS / 64][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j = blockIdx.x * (STITCH_THREADS / 64) + wid;
  const bool live = j < a.J;
  bool finite = true;
  if (live && lane < C * C) {
    double s = 0.0;
    if (j > 0) {
      const double* pp = a.part + (long)(j - 1) * a.nchunk * (C * C) + lane;
      for (int ch = 0; ch < a.nchunk; ++ch) s += pp[(long)ch * (C * C)];
    }
    a.sim[(long)j * (C * C) + lane] = s;
    sS[wid][lane] = s;
    finite = isfinite(s);
  }
  __syncthreads();
  if (!live) return;
  const bool bad = __ballot(!finite) != 0ull;
  constexpr int NP = Fact<C>::v;
  double best = 0.0;
  int bestk = NP;   // NP: this lane has scored nothing
  if (j > 0 && !bad) {
    for (int k = lane; k < NP; k += 64) {
      double sc;
      stitch_kth_perm<C>(k, sS[wid], &sc);
      if (bestk == NP || sc > best) { best = sc; bestk = k; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int ok = __shfl_xor(bestk, o, 64);
      if (ok != NP && (bestk == NP || ob > best || (ob == best && ok < bestk))) { best = ob; bestk = ok; }
    }
  } else {
    bestk = 0;
  }
  const uint32_t pk = stitch_kth_perm<C>(bestk, nullptr, nullptr);
  if (lane < C) a.perm[(long)j * C + lane] = (int32_t)((pk >> (4 * lane)) & 15u);
  if (lane == 0) a.status[j] = (j > 0 && bad) ? 1 : 0;
}

// ---------------------------------------------------------------------------
// chain: sigma_0 = id, sigma_j(c) = pi_j(sigma_{j-1}(c)): an inclusive scan of the boundary
// permutations under composition, on nibble-packed permutations.  One workgroup walks the
// windows 256 at a time: a shuffle scan inside each wave, the wave totals through LDS, and
// the running prefix carried from tile to tile.  Composition is exact, so the grouping
// does not matter.
// ---------------------------------------------------------------------------
// (x then y)(c) = y(x(c))
template <int C> CTN_DEV uint32_t stitch_compose(uint32_t x, uint32_t y) {
  uint32_t r = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const uint32_t xc = (x >> (4 * c)) & 7u;
    r |= ((y >> (4 * xc)) & 7u) << (4 * c);
  }
  return r;
}

template <int C> __global__ __launch_bounds__(STITCH_THREADS) void stitch_chain_kernel(StitchArgs a) {
  __shared__ uint32_t tot[STITCH_THREADS / 64];
  constexpr uint32_t ID = 0x76543210u;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  uint32_t carry = ID;
  for (long base = 0; base < a.J; base += STITCH_THREADS) {
    const long j = base + tid;
    uint32_t x = ID;
    if (j < a.J) {
      x = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const uint32_t v = (uint32_t)a.perm[j * C + c];
        x |= (v < (uint32_t)C ? v : (uint32_t)c) << (4 * c);
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = __shfl_up(x, d, 64);
      if (lane >= d) x = stitch_compose<C>(y, x);
    }
    if (lane == 63) tot[wid] = x;
    __syncthreads();
    uint32_t pre = carry;
    for (int w = 0; w < wid; ++w) pre = stitch_compose<C>(pre, tot[w]);
    x = stitch_compose<C>(pre, x);
    for (int w = 0; w < STITCH_THREADS / 64; ++w) carry = stitch_compose<C>(carry, tot[w]);
    if (j < a.J) {
#pragma unroll
      for (int c = 0; c < C; ++c) a.sigma[j * C + c] = (int32_t)((x >> (4 * c)) & 7u);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// overlap-add: out[c][t], t < T.  Window j = min(t / Hs, J - 1), u = t - j Hs; for j >= 1 and
// u < O the sample is the cross-fade of window j-1 at Hs + u and window j at u, each read
// through its own sigma; elsewhere a copy.  Separate multiply, subtract and add, each
// rounded to nearest: no contraction.
// ---------------------------------------------------------------------------
CTN_DEV float stitch_fade(float f, float p, float c) {
  return (1.f - f) * p + f * c;
}
CTN_DEV int stitch_sigma(const StitchArgs& a, int j, int c) {
  const uint32_t s = (uint32_t)a.sigma_in[(long)j * a.C + c];
  return s < (uint32_t)a.C ? (int)s : c;
}
CTN_DEV float stitch_sample(const StitchArgs& a, int c, long t) {
  long j = t / a.Hs;
  if (j > a.J - 1) j = a.J - 1;
  const long u = t - j * a.Hs;
  const float cv = a.P[((long)j * a.C + stitch_sigma(a, (int)j, c)) * a.W + u];
  if (j == 0 || u >= a.O) return cv;
  const float pv = a.P[((long)(j - 1) * a.C + stitch_sigma(a, (int)j - 1, c)) * a.W + a.Hs + u];
  return stitch_fade(a.fade[u], pv, cv);
}

template <bool VEC, bool VEC_OUT> __global__ __launch_bounds__(STITCH_THREADS) void stitch_ola_kernel(StitchArgs a) {
  const int c = blockIdx.y;
  const long t0 = 4 * ((long)blockIdx.x * STITCH_THREADS + threadIdx.x);
  if (t0 >= a.T) return;
  float* dst = a.out + (long)c * a.T + t0;
  if (VEC && t0 + 3 < a.T) {
    // W, O and Hs are multiples of 4: the four samples share j and the side of the fade
    long j = t0 / a.Hs;
    if (j > a.J - 1) j = a.J - 1;
    const long u = t0 - j * a.Hs;
    float4 v = *reinterpret_cast<const float4*>(a.P + ((long)j * a.C + stitch_sigma(a, (int)j, c)) * a.W + u);
    if (j > 0 && u < a.O) {
      const float4 p =
          *reinterpret_cast<const float4*>(a.P + ((long)(j - 1) * a.C + stitch_sigma(a, (int)j - 1, c)) * a.W + a.Hs + u);
      const float4 f = *reinterpret_cast<const float4*>(a.fade + u);
      v.x = stitch_fade(f.x, p.x, v.x);
      v.y = stitch_fade(f.y, p.y, v.y);
      v.z = stitch_fade(f.z, p.z, v.z);
      v.w = stitch_fade(f.w, p.w, v.w);
    }
    if (VEC_OUT) {
      *reinterpret_cast<float4*>(dst) = v;
    } else {
      dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (t0 + e < a.T) dst[e] = stitch_sample(a, c, t0 + e);
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_stitch_frame(const StitchArgs& a, hipStream_t s) {
  const long per = (a.W + 4 * STITCH_THREADS - 1) / (4 * STITCH_THREADS);
  const dim3 grid((unsigned)(per * a.J)), blk(STITCH_THREADS);
  if (a.vec) stitch_frame_kernel<true><<<grid, blk, 0, s>>>(a);
  else stitch_frame_kernel<false><<<grid, blk, 0, s>>>(a);
  return hipGetLastError();
}

template <int C> static void stitch_plan_c(const StitchArgs& a, hipStream_t s) {
  const dim3 blk(STITCH_THREADS);
  if (a.J > 1) {
    const dim3 grid((unsigned)((long)(a.J - 1) * a.nchunk));
    if (a.vec) stitch_corr_kernel<C, true><<<grid, blk, 0, s>>>(a);
    else stitch_corr_kernel<C, false><<<grid, blk, 0, s>>>(a);
  }
  constexpr int wpb = STITCH_THREADS / 64;
  stitch_perm_kernel<C><<<dim3((unsigned)((a.J + wpb - 1) / wpb)), blk, 0, s>>>(a);
  stitch_chain_kernel<C><<<dim3(1), blk, 0, s>>>(a);
}

hipError_t launch_stitch_plan(const StitchArgs& a, hipStream_t s) {
  switch (a.C) {
    case 2: stitch_plan_c<2>(a, s); break;
    case 3: stitch_plan_c<3>(a, s); break;
    case 4: stitch_plan_c<4>(a, s); break;
    case 5: stitch_plan_c<5>(a, s); break;
    case 6: stitch_plan_c<6>(a, s); break;
    case 7: stitch_plan_c<7>(a, s); break;
    case 8: stitch_plan_c<8>(a, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_stitch_ola(const StitchArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.T + 4L * STITCH_THREADS - 1) / (4L * STITCH_THREADS)), (unsigned)a.C), blk(STITCH_THREADS);
  if (a.vec && a.vec_out) stitch_ola_kernel<true, true><<<grid, blk, 0, s>>>(a);
  else if (a.vec) stitch_ola_kernel<true, false><<<grid, blk, 0, s>>>(a);
  else stitch_ola_kernel<false, false><<<grid, blk, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace ctn
