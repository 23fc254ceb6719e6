// Dynamic mixing with reverberation and noise (include/ctn.h: ctn_dmix_draw_aug,
// ctn_dmix_mix_aug).
//
// draw  : one thread per row: the RIR index of every slot and the row's noise entry, from
//         Philox counters (g_lo, g_hi, 16 + c, 0) and (g_lo, g_hi, 32, 0); the source plan and
//         the speed indices come from launch_dmix_draw.
// reverb: xv[n] = sum_{j <= min(n, L - 1)} h[j] xs[n - j], j upward, acc = fl32(acc + fl32(h x))
//         from +0, of every slot into the workspace, with the tables that present xv to the mix
//         kernels as an fp32 pool (as the resampler does).  A workgroup of 256 threads covers
//         DMIX_CHUNK outputs, thread t the 8 consecutive outputs n0 + 8 t ... n0 + 8 t + 7, whose
//         sums it carries in registers over the tap tiles.  A tile stages DMIX_RIR_TILE taps and
//         the DMIX_CHUNK + DMIX_RIR_TILE input samples under them in LDS (12 KiB whatever L is).
//         Per 4 taps a thread reads the 4 taps (one 16-byte broadcast read) and the 4 next-older
//         inputs (one 16-byte read) and does 32 multiplies and 32 adds on a 12-sample register
//         window.  Inputs before the segment's first sample are staged as +0: the sum starts at
//         +0 and a sum of two zeros of unlike sign is +0, so adding fl32(h * 0) = +-0 equals
//         skipping the term; the same holds for the zero taps that pad L to a multiple of 4.
// noise : power (per-chunk fp64 sums of s^2 and z^2), ngain (one thread per row: the row's
//         noise validity and g_z), then the peak and write stages of ctn_dmix.hip with the noise
//         term added last.
// No atomics; every sum and max is finished in index order.
#pragma clang fp contract(off)

#include "ctn_common.h"
#include "ctn_dmix_aug.h"
#include "ctn_dmix_dev.h"

namespace ctn {

static_assert(DMIX_CHUNK == 256 * DMIX_RIR_OUT && DMIX_RIR_OUT == 8, "a workgroup covers one chunk, 8 outputs per thread");
static_assert(DMIX_RIR_TILE % 256 == 0 && DMIX_RIR_TILE % 4 == 0, "tap tile");

DmixAugLayout dmix_aug_layout(int M, int C, int T, bool speeds, bool rirs, bool noise) {
  DmixAugLayout L{};
  if (speeds) {
    L.sp = dmix_sp_layout(M, C, T);
  } else {
    L.sp.mix = dmix_layout(M, C, T);
    L.sp.bytes = L.sp.mix.bytes;
  }
  const size_t mc = (size_t)M * C;
  size_t o = L.sp.bytes;
  if (rirs || noise) o = (o + 15) / 16 * 16;
  if (rirs) {
    L.off_xv = o;    o += (mc * (size_t)T * sizeof(float) + 15) / 16 * 16;
    L.off_vplan = o; o += mc * sizeof(DmixEntry);
    L.off_voff = o;  o += ((mc + 1) * sizeof(int64_t) + 15) / 16 * 16;
  }
  if (noise) {
    L.off_pw = o;  o += (size_t)M * L.sp.mix.nchunk * 2 * sizeof(double);
    L.off_ng0 = o; o += ((size_t)M * sizeof(float) + 15) / 16 * 16;
  }
  L.bytes = o;
  return L;
}

// ---------------------------------------------------------------------------
// draw
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void dmix_draw_aug_kernel(DmixAugDrawArgs a) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= a.M) return;
  const uint64_t g = (uint64_t)((a.first_dev ? *a.first_dev : a.first) + m);
  if (a.rir) {
    for (int c = 0; c < a.C; ++c) {
      const Philox r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)(16 + c), 0u, a.seed_lo, a.seed_hi);
      const float u = (float)(r.r[1] >> 8) * 0x1p-24f;
      a.rir[(size_t)m * a.C + c] =
          (a.n_rirs > 0 && u < a.rir_prob) ? (int32_t)(((uint64_t)r.r[0] * (uint64_t)a.n_rirs) >> 32) : -1;
    }
  }
  if (a.nplan) {
    const Philox r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 32u, 0u, a.seed_lo, a.seed_hi);
    const float u = (float)(r.r[2] >> 8) * 0x1p-24f;
    DmixEntry e{-1, 0, a.snr_lo + (a.snr_hi - a.snr_lo) * u, 1};
    const int32_t utt = a.nelig[((uint64_t)r.r[0] * (uint64_t)a.NE) >> 32];
    if (utt >= 0 && utt < a.NU) {
      const int64_t n = a.noff[utt + 1] - a.noff[utt] - a.T + 1;
      if (n >= 1 && n <= 0x7fffffffLL) {
        e.utt = utt;
        e.start = (int32_t)(((uint64_t)r.r[1] * (uint64_t)n) >> 32);
      }
    }
    a.nplan[m] = e;
  }
}

hipError_t launch_dmix_draw_aug(const DmixAugDrawArgs& a, hipStream_t s) {
  dmix_draw_aug_kernel<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// reverberation
// ---------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));

template <int DT> CTN_DEV float sample(const void* pool, int64_t i) {
  if constexpr (DT == 0) return (float)reinterpret_cast<const int16_t*>(pool)[i] * 0x1p-15f;
  else return reinterpret_cast<const float*>(pool)[i];
}

// First pool sample of the entry's segment of T samples, or -1 for an entry that must not be read.
CTN_DEV int64_t entry_base(const int64_t* off, int U, int T, const DmixEntry& e) {
  if (e.utt < 0 || e.utt >= U || e.start < 0) return -1;
  const int64_t o = off[e.utt], len = off[e.utt + 1] - o;
  if ((int64_t)e.start + T > len) return -1;
  return o + e.start;
}

// grid: (m*C + c) * nchunk + chunk
template <int DT> __global__ __launch_bounds__(256) void dmix_reverb_kernel(DmixReverbArgs a) {
  __shared__ __attribute__((aligned(16))) float xw[DMIX_CHUNK + DMIX_RIR_TILE];
  __shared__ __attribute__((aligned(16))) float hs[DMIX_RIR_TILE];
  const int nchunk = a.L.sp.mix.nchunk;
  const int mc = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  const int tid = threadIdx.x;
  const DmixEntry e = a.plan[mc];
  const int32_t k = a.rir[mc];
  const int64_t sbase = entry_base(a.off, a.U, a.T, e);
  bool ok = sbase >= 0 && k >= -1 && k < a.n_rirs;
  int64_t ho = 0;
  int taps = 0;
  if (ok && k >= 0) {
    ho = a.roff[k];
    const int64_t l = a.roff[k + 1] - ho;
    ok = l >= 1 && l <= a.max_taps;
    taps = (int)l;
  }
  if (chunk == 0 && tid == 0) {   // the tables that present xv to the mix kernels
    reinterpret_cast<DmixEntry*>(a.ws + a.L.off_vplan)[mc] = DmixEntry{ok ? mc : -1, 0, e.level_db, e.tries};
    int64_t* off2 = reinterpret_cast<int64_t*>(a.ws + a.L.off_voff);
    off2[mc] = (int64_t)mc * a.T;
    if (mc == a.M * a.C - 1) off2[mc + 1] = (int64_t)(mc + 1) * a.T;
  }
  if (!ok) return;                // utt = -1 above: the mix kernels never read this row of xv
  float* xv = reinterpret_cast<float*>(a.ws + a.L.off_xv) + (size_t)mc * a.T;
  const int n0 = chunk * DMIX_CHUNK, t0 = n0 + tid * 8;
  if (k < 0) {                    // dry: exact copy
    float x[8];
    load8<DT>(a.pool, sbase, t0, a.T, x);
    store8(xv, t0, a.T, x);
    return;
  }
  const int nlast = min(n0 + DMIX_CHUNK, a.T) - 1;   // the chunk's last output: taps j > nlast meet no input
  const int jend = min(taps, nlast + 1);
  float acc[8] = {};
  for (int j0 = 0; j0 < jend; j0 += DMIX_RIR_TILE) {
    if (j0) __syncthreads();      // the previous tile has been consumed
    for (int t = tid; t < DMIX_RIR_TILE; t += 256) hs[t] = j0 + t < taps ? a.rir_pool[ho + j0 + t] : 0.f;
    // xw[i] = xs[n0 - j0 - TILE + i]; +0 outside the segment, which is never read
    const int64_t nw = (int64_t)n0 - j0 - DMIX_RIR_TILE;
    for (int i = tid; i < DMIX_CHUNK + DMIX_RIR_TILE; i += 256) {
      const int64_t n = nw + i;
      xw[i] = (n >= 0 && n < a.T) ? sample<DT>(a.pool, sbase + n) : 0.f;
    }
    __syncthreads();
    const int jn = (min(jend - j0, DMIX_RIR_TILE) + 3) & ~3;
    // w[4 + r] = xs[t0 + r - j] for the tile's tap jj = j - j0; w[0..3] the 4 next-older inputs
    const float* xt = xw + DMIX_RIR_TILE + tid * 8;
    float w[12];
    {
      const v4f lo = *reinterpret_cast<const v4f*>(xt), hi = *reinterpret_cast<const v4f*>(xt + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        w[4 + i] = lo[i];
        w[8 + i] = hi[i];
      }
    }
#pragma unroll 2
    for (int jj = 0; jj < jn; jj += 4) {
      const v4f h4 = *reinterpret_cast<const v4f*>(hs + jj);
      const v4f x4 = *reinterpret_cast<const v4f*>(xt - jj - 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) w[i] = x4[i];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = acc[r] + h4[t] * w[4 + r - t];
#pragma unroll
      for (int i = 11; i >= 4; --i) w[i] = w[i - 4];
    }
  }
  store8(xv, t0, a.T, acc);
}

hipError_t launch_dmix_reverb(const DmixReverbArgs& r, DmixMixArgs* mix, hipStream_t s) {
  const unsigned segs = (unsigned)((long)r.M * r.C * r.L.sp.mix.nchunk);
  if (r.pool_dtype == 0) dmix_reverb_kernel<0><<<dim3(segs), dim3(256), 0, s>>>(r);
  else dmix_reverb_kernel<1><<<dim3(segs), dim3(256), 0, s>>>(r);
  mix->U = r.M * r.C;
  mix->pool_dtype = 1;
  mix->pool = r.ws + r.L.off_xv;
  mix->off = reinterpret_cast<const int64_t*>(r.ws + r.L.off_voff);
  mix->plan = reinterpret_cast<const DmixEntry*>(r.ws + r.L.off_vplan);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// noise: power, gain, then the peak and write stages with the noise term added last
// ---------------------------------------------------------------------------
CTN_DEV void row_tables(const DmixMixArgs& a, int m, int64_t* base, float* g) {
  if ((int)threadIdx.x < a.C) {
    base[threadIdx.x] = seg_base(a, a.plan[(size_t)m * a.C + threadIdx.x]);
    g[threadIdx.x] = reinterpret_cast<const float*>(a.ws + a.L.off_g0)[(size_t)m * a.C + threadIdx.x];
  }
}

// grid: m * nchunk + chunk
template <int DT, int NDT> __global__ __launch_bounds__(256) void dmix_power_kernel(DmixMixArgs a, DmixNoiseArgs nz) {
  __shared__ double red[8];
  __shared__ int64_t base[DMIX_MAX_C];
  __shared__ float g[DMIX_MAX_C];
  const int nchunk = a.L.nchunk;
  const int m = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  double* out = reinterpret_cast<double*>(a.ws + nz.off_pw) + ((size_t)m * nchunk + chunk) * 2;
  const int64_t nb = entry_base(nz.off, nz.NU, a.T, nz.nplan[m]);
  if (a.status[m] != 0 || nb < 0) {
    if (threadIdx.x == 0) out[0] = out[1] = 0.0;
    return;
  }
  row_tables(a, m, base, g);
  __syncthreads();
  const int t0 = chunk * DMIX_CHUNK + (int)threadIdx.x * 8;
  float acc[8], z[8];
  mix8<DT>(a, base, g, t0, acc, nullptr);
  load8<NDT>(nz.pool, nb, t0, a.T, z);
  double s[2] = {0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 8; ++i) {   // samples past T are zeros
    s[0] += (double)acc[i] * (double)acc[i];
    s[1] += (double)z[i] * (double)z[i];
  }
  block_sum_d<2>(s, red);
  if (threadIdx.x == 0) {
    out[0] = s[0];
    out[1] = s[1];
  }
}

__global__ __launch_bounds__(64) void dmix_ngain_kernel(DmixMixArgs a, DmixNoiseArgs nz) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= a.M) return;
  float* ng0 = reinterpret_cast<float*>(a.ws + nz.off_ng0);
  const DmixEntry e = nz.nplan[m];
  if (a.status[m] != 0 || entry_base(nz.off, nz.NU, a.T, e) < 0) {
    a.status[m] = 1;
    float* g0 = reinterpret_cast<float*>(a.ws + a.L.off_g0) + (size_t)m * a.C;
    for (int c = 0; c < a.C; ++c) g0[c] = 0.f;
    ng0[m] = 0.f;
    return;
  }
  const double* pw = reinterpret_cast<const double*>(a.ws + nz.off_pw) + (size_t)m * a.L.nchunk * 2;
  double ps = 0.0, pz = 0.0;
  for (int k = 0; k < a.L.nchunk; ++k) {
    ps += pw[2 * k];
    pz += pw[2 * k + 1];
  }
  ps /= (double)a.T;
  pz /= (double)a.T;
  ng0[m] = (float)(sqrt(ps / fmax(pz, 1e-8)) * exp10(-(double)e.level_db / 20.0));
}

// grid: m * nchunk + chunk
template <int DT, int NDT> __global__ __launch_bounds__(256) void dmix_peak_noise_kernel(DmixMixArgs a, DmixNoiseArgs nz) {
  __shared__ float red[4];
  __shared__ int64_t base[DMIX_MAX_C];
  __shared__ float g[DMIX_MAX_C];
  const int nchunk = a.L.nchunk;
  const int m = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  float* out = reinterpret_cast<float*>(a.ws + a.L.off_pmax) + (size_t)m * nchunk + chunk;
  if (a.status[m] != 0) {
    if (threadIdx.x == 0) *out = 0.f;
    return;
  }
  row_tables(a, m, base, g);
  __syncthreads();
  const int t0 = chunk * DMIX_CHUNK + (int)threadIdx.x * 8;
  const float gz = reinterpret_cast<const float*>(a.ws + nz.off_ng0)[m];
  float acc[8], z[8];
  mix8<DT>(a, base, g, t0, acc, nullptr);
  load8<NDT>(nz.pool, entry_base(nz.off, nz.NU, a.T, nz.nplan[m]), t0, a.T, z);
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float v = gz * z[i];
    p = fmaxf(p, fabsf(acc[i] + v));
  }
  p = block_max(p, red);
  if (threadIdx.x == 0) *out = p;
}

// grid: m * nchunk + chunk
template <int DT, int NDT> __global__ __launch_bounds__(256) void dmix_write_noise_kernel(DmixMixArgs a, DmixNoiseArgs nz) {
  __shared__ int64_t base[DMIX_MAX_C];
  __shared__ float g[DMIX_MAX_C + 1];
  const int nchunk = a.L.nchunk;
  const int m = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  const int t0 = chunk * DMIX_CHUNK + (int)threadIdx.x * 8;
  float* src0 = a.sources + (size_t)m * a.C * a.T;
  float* mixrow = a.mixture + (size_t)m * a.T;
  float* nrow = nz.noise_out ? nz.noise_out + (size_t)m * a.T : nullptr;
  if (a.status[m] != 0) {
    const float z[8] = {};
    for (int c = 0; c < a.C; ++c) store8(src0 + (size_t)c * a.T, t0, a.T, z);
    store8(mixrow, t0, a.T, z);
    if (nrow) store8(nrow, t0, a.T, z);
    if (chunk == 0 && (int)threadIdx.x < a.C) a.gains[(size_t)m * a.C + threadIdx.x] = 0.f;
    if (chunk == 0 && threadIdx.x == 0) nz.ngain[m] = 0.f;
    return;
  }
  if ((int)threadIdx.x <= a.C) {   // thread C: the noise gain
    const int c = threadIdx.x;
    const bool noise = c == a.C;
    if (!noise) base[c] = seg_base(a, a.plan[(size_t)m * a.C + c]);
    float gc = noise ? reinterpret_cast<const float*>(a.ws + nz.off_ng0)[m]
                     : reinterpret_cast<const float*>(a.ws + a.L.off_g0)[(size_t)m * a.C + c];
    if (a.peak > 0.f) {
      const float* pm = reinterpret_cast<const float*>(a.ws + a.L.off_pmax) + (size_t)m * nchunk;
      float p = 0.f;
      for (int k = 0; k < nchunk; ++k) p = fmaxf(p, pm[k]);
      if (p > a.peak) gc = gc * (a.peak / p);
    }
    g[c] = gc;
    if (chunk == 0) {
      if (noise) nz.ngain[m] = gc;
      else a.gains[(size_t)m * a.C + c] = gc;
    }
  }
  __syncthreads();
  float acc[8], z[8];
  mix8<DT>(a, base, g, t0, acc, src0);
  load8<NDT>(nz.pool, entry_base(nz.off, nz.NU, a.T, nz.nplan[m]), t0, a.T, z);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    z[i] = g[a.C] * z[i];
    acc[i] = acc[i] + z[i];
  }
  store8(mixrow, t0, a.T, acc);
  if (nrow) store8(nrow, t0, a.T, z);
}

template <int DT, int NDT> static void mix_noise_stages(const DmixMixArgs& a, const DmixNoiseArgs& nz, hipStream_t s) {
  const dim3 blk(256), rows((unsigned)((long)a.M * a.L.nchunk));
  dmix_power_kernel<DT, NDT><<<rows, blk, 0, s>>>(a, nz);
  dmix_ngain_kernel<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a, nz);
  if (a.peak > 0.f) dmix_peak_noise_kernel<DT, NDT><<<rows, blk, 0, s>>>(a, nz);
  dmix_write_noise_kernel<DT, NDT><<<rows, blk, 0, s>>>(a, nz);
}

hipError_t launch_dmix_mix_noise(const DmixMixArgs& a, const DmixNoiseArgs& nz, hipStream_t s) {
  if (hipError_t e = launch_dmix_gain0(a, s); e != hipSuccess) return e;
  if (a.pool_dtype == 0) {
    if (nz.dtype == 0) mix_noise_stages<0, 0>(a, nz, s);
    else mix_noise_stages<0, 1>(a, nz, s);
  } else {
    if (nz.dtype == 0) mix_noise_stages<1, 0>(a, nz, s);
    else mix_noise_stages<1, 1>(a, nz, s);
  }
  return hipGetLastError();
}

}  // namespace ctn
