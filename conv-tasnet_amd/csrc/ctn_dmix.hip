// Dynamic mixing on the device (include/ctn.h: ctn_dmix_draw, ctn_dmix_mix, ctn_dmix_draw_sp,
// ctn_dmix_mix_sp).
//
// draw : one thread per batch row; Philox4x32-10 counter (g_lo, g_hi, slot, try), key = seed.
// mix  : ssq   (level_mode 1) per-chunk sums of squares of every segment, fp64
//        gain0 one thread per row: validity, status, gains before the guard
//        peak  (peak > 0) per-chunk max |sum_c fl32(g_c x_c)| of every row
//        write final gains, sources, mixture
// mix_sp: resample (every segment through its speed's polyphase FIR into the workspace),
//        then the mix kernels above on the resampled segments
// A workgroup of 256 threads covers DMIX_CHUNK = 2048 consecutive samples of one segment
// (ssq) or one row (peak, write), 8 per thread.  A segment starts at any sample of the pool,
// so an int16 segment at any 2-byte and the fp32 rows (T is arbitrary) at any 4-byte
// alignment: the 16-byte accesses are declared with that alignment (global memory on
// gfx950 is accessed in unaligned mode) and cover exactly the thread's 8 samples, never a
// byte outside the segment or the row; a last partial group of 8 goes sample by sample.
// The device helpers shared with ctn_dmix_aug.hip (reverberation and noise) are in ctn_dmix_dev.h.
// No atomics; every sum and max is finished in index order.  The exactness contract
// (one rounding per source sample, the mixture an ordered fp32 sum of the stored sources)
// needs every product and sum below to stay a separate operation:
#pragma clang fp contract(off)

#include "ctn_common.h"
#include "ctn_dmix.h"
#include "ctn_dmix_dev.h"

namespace ctn {

static_assert(sizeof(DmixEntry) == 16, "plan entry is 16 bytes");
static_assert(DMIX_CHUNK == 256 * 8, "a workgroup covers one chunk");

DmixLayout dmix_layout(int M, int C, int T) {
  DmixLayout L{};
  L.nchunk = (int)(((long)T + DMIX_CHUNK - 1) / DMIX_CHUNK);
  const size_t mc = (size_t)M * C;
  size_t o = 0;
  L.off_ssq = o;  o += mc * L.nchunk * sizeof(double);
  L.off_g0 = o;   o += (mc * sizeof(float) + 15) / 16 * 16;
  L.off_pmax = o; o += ((size_t)M * L.nchunk * sizeof(float) + 15) / 16 * 16;
  L.bytes = o;
  return L;
}

// ---------------------------------------------------------------------------
// draw
// ---------------------------------------------------------------------------
// SP: the slot's speed index k = (r3 * S) >> 32 is drawn first and the segment needs span[k]
// input samples instead of T (ctn_dmix_draw_sp); one entry of ratio 1/1 gives the plain plan.
template <bool SP> __global__ __launch_bounds__(64) void dmix_draw_kernel(DmixDrawArgs a) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= a.M) return;
  const uint64_t g = (uint64_t)((a.first_dev ? *a.first_dev : a.first) + m);
  int32_t taken[DMIX_MAX_C];   // speakers of the accepted slots; bit q of `valid`: slot q has one
  uint32_t valid = 0;
  for (int c = 0; c < a.C; ++c) {
    DmixEntry e{-1, 0, 0.f, 0};
    int32_t sp = 0, k = 0;
    for (int j = 0; j < a.max_tries; ++j) {
      const Philox r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)c, (uint32_t)j, a.seed_lo, a.seed_hi);
      int64_t need = a.T;
      if constexpr (SP) {
        k = (int32_t)(((uint64_t)r.r[3] * (uint64_t)a.nspeed) >> 32);
        need = a.span[k];
      }
      const int32_t utt = a.elig[((uint64_t)r.r[0] * (uint64_t)a.E) >> 32];
      const float u = (float)(r.r[2] >> 8) * 0x1p-24f;
      e.level_db = a.lo_db + (a.hi_db - a.lo_db) * u;
      e.tries = j + 1;
      e.utt = -1;
      e.start = 0;
      if (utt < 0 || utt >= a.U) break;                    // a bad table entry: flagged by the mix
      const int64_t n = a.off[utt + 1] - a.off[utt] - need + 1;
      if (n < 1 || n > 0x7fffffffLL) break;
      e.utt = utt;
      e.start = (int32_t)(((uint64_t)r.r[1] * (uint64_t)n) >> 32);
      sp = a.spk[utt];
      bool clash = false;
      for (int q = 0; q < c; ++q) clash = clash || (((valid >> q) & 1u) && taken[q] == sp);
      if (!clash) break;
    }
    taken[c] = sp;
    if (e.utt >= 0) valid |= 1u << c;
    a.plan[(size_t)m * a.C + c] = e;
    if constexpr (SP) a.speed[(size_t)m * a.C + c] = k;
  }
}

__global__ void dmix_advance_kernel(int64_t* first, int64_t advance) { *first += advance; }

hipError_t launch_dmix_draw(const DmixDrawArgs& a, hipStream_t s) {
  if (a.speed) dmix_draw_kernel<true><<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
  else dmix_draw_kernel<false><<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
  if (a.first_dev) dmix_advance_kernel<<<dim3(1), dim3(1), 0, s>>>(a.first_dev, a.advance);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// thin: how many of a row's slots speak (ctn_dmix_thin)
// ---------------------------------------------------------------------------
// One thread per row: n_m = min + ((r0 (C - min + 1)) >> 32) from the row's own Philox draw;
// slots c >= n_m get level_db = -inf, which the gain stage turns into a gain of exactly 0.
__global__ __launch_bounds__(64) void dmix_thin_kernel(DmixThinArgs a) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= a.M) return;
  const uint64_t g = (uint64_t)((a.first_dev ? *a.first_dev - a.back : a.first) + m);
  const Philox r = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), DMIX_COUNT_SLOT, 0u, a.seed_lo, a.seed_hi);
  const int n = a.min_speakers + (int)(((uint64_t)r.r[0] * (uint64_t)(a.C - a.min_speakers + 1)) >> 32);
  for (int c = n; c < a.C; ++c) a.plan[(size_t)m * a.C + c].level_db = -INFINITY;
  a.count[m] = n;
}

hipError_t launch_dmix_thin(const DmixThinArgs& a, hipStream_t s) {
  dmix_thin_kernel<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// mix
// ---------------------------------------------------------------------------
// grid: (m*C + c) * nchunk + chunk
template <int DT> __global__ __launch_bounds__(256) void dmix_ssq_kernel(DmixMixArgs a) {
  __shared__ double red[4];
  const int nchunk = a.L.nchunk;
  const int mc = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  double* out = reinterpret_cast<double*>(a.ws + a.L.off_ssq) + (size_t)mc * nchunk + chunk;
  const int64_t base = seg_base(a, a.plan[mc]);
  if (base < 0) {
    if (threadIdx.x == 0) *out = 0.0;
    return;
  }
  float x[8];
  load8<DT>(a.pool, base, chunk * DMIX_CHUNK + (int)threadIdx.x * 8, a.T, x);
  double s[1] = {0.0};
#pragma unroll
  for (int i = 0; i < 8; ++i) s[0] += (double)x[i] * (double)x[i];
  block_sum_d<1>(s, red);
  if (threadIdx.x == 0) *out = s[0];
}

__global__ __launch_bounds__(64) void dmix_gain0_kernel(DmixMixArgs a) {
  const int m = blockIdx.x * 64 + threadIdx.x;
  if (m >= a.M) return;
  bool ok = true;
  for (int c = 0; c < a.C; ++c) ok = ok && seg_base(a, a.plan[(size_t)m * a.C + c]) >= 0;
  a.status[m] = ok ? 0 : 1;
  float* g0 = reinterpret_cast<float*>(a.ws + a.L.off_g0) + (size_t)m * a.C;
  const double* ssq = reinterpret_cast<const double*>(a.ws + a.L.off_ssq);
  for (int c = 0; c < a.C; ++c) {
    if (!ok) {
      g0[c] = 0.f;
      continue;
    }
    double g = exp10((double)a.plan[(size_t)m * a.C + c].level_db / 20.0);
    if (a.level_mode == 1) {
      double s = 0.0;
      for (int k = 0; k < a.L.nchunk; ++k) s += ssq[((size_t)m * a.C + c) * a.L.nchunk + k];
      g /= fmax(sqrt(s / (double)a.T), 1e-4);
    }
    g0[c] = (float)g;
  }
}

// grid: m * nchunk + chunk
template <int DT> __global__ __launch_bounds__(256) void dmix_peak_kernel(DmixMixArgs a) {
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
  if ((int)threadIdx.x < a.C) {
    base[threadIdx.x] = seg_base(a, a.plan[(size_t)m * a.C + threadIdx.x]);
    g[threadIdx.x] = reinterpret_cast<const float*>(a.ws + a.L.off_g0)[(size_t)m * a.C + threadIdx.x];
  }
  __syncthreads();
  float acc[8];
  mix8<DT>(a, base, g, chunk * DMIX_CHUNK + (int)threadIdx.x * 8, acc, nullptr);
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) p = fmaxf(p, fabsf(acc[i]));   // samples past T are zeros
  p = block_max(p, red);
  if (threadIdx.x == 0) *out = p;
}

// grid: m * nchunk + chunk
template <int DT> __global__ __launch_bounds__(256) void dmix_write_kernel(DmixMixArgs a) {
  __shared__ int64_t base[DMIX_MAX_C];
  __shared__ float g[DMIX_MAX_C];
  const int nchunk = a.L.nchunk;
  const int m = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  const int t0 = chunk * DMIX_CHUNK + (int)threadIdx.x * 8;
  float* src0 = a.sources + (size_t)m * a.C * a.T;
  float* mixrow = a.mixture + (size_t)m * a.T;
  if (a.status[m] != 0) {
    const float z[8] = {};
    for (int c = 0; c < a.C; ++c) store8(src0 + (size_t)c * a.T, t0, a.T, z);
    store8(mixrow, t0, a.T, z);
    if (chunk == 0 && (int)threadIdx.x < a.C) a.gains[(size_t)m * a.C + threadIdx.x] = 0.f;
    return;
  }
  if ((int)threadIdx.x < a.C) {
    const int c = threadIdx.x;
    base[c] = seg_base(a, a.plan[(size_t)m * a.C + c]);
    float gc = reinterpret_cast<const float*>(a.ws + a.L.off_g0)[(size_t)m * a.C + c];
    if (a.peak > 0.f) {
      const float* pm = reinterpret_cast<const float*>(a.ws + a.L.off_pmax) + (size_t)m * nchunk;
      float p = 0.f;
      for (int k = 0; k < nchunk; ++k) p = fmaxf(p, pm[k]);
      if (p > a.peak) gc = gc * (a.peak / p);
    }
    g[c] = gc;
    if (chunk == 0) a.gains[(size_t)m * a.C + c] = gc;
  }
  __syncthreads();
  float acc[8];
  mix8<DT>(a, base, g, t0, acc, src0);
  store8(mixrow, t0, a.T, acc);
}

hipError_t launch_dmix_gain0(const DmixMixArgs& a, hipStream_t s) {
  const dim3 blk(256), segs((unsigned)((long)a.M * a.C * a.L.nchunk));
  if (a.level_mode == 1) {
    if (a.pool_dtype == 0) dmix_ssq_kernel<0><<<segs, blk, 0, s>>>(a);
    else dmix_ssq_kernel<1><<<segs, blk, 0, s>>>(a);
  }
  dmix_gain0_kernel<<<dim3((a.M + 63) / 64), dim3(64), 0, s>>>(a);
  return hipGetLastError();
}

hipError_t launch_dmix_mix(const DmixMixArgs& a, hipStream_t s) {
  const int nchunk = a.L.nchunk;
  const dim3 blk(256), rows((unsigned)((long)a.M * nchunk));
  const bool i16 = a.pool_dtype == 0;
  if (hipError_t e = launch_dmix_gain0(a, s); e != hipSuccess) return e;
  if (a.peak > 0.f) {
    if (i16) dmix_peak_kernel<0><<<rows, blk, 0, s>>>(a);
    else dmix_peak_kernel<1><<<rows, blk, 0, s>>>(a);
  }
  if (i16) dmix_write_kernel<0><<<rows, blk, 0, s>>>(a);
  else dmix_write_kernel<1><<<rows, blk, 0, s>>>(a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// speed perturbation: polyphase resampling of every segment, then the mix above
// ---------------------------------------------------------------------------
static_assert(DMIX_SP_WINDOW % 8 == 0 && DMIX_SP_WINDOW >= 2 * (DMIX_CHUNK - 1) + 40 + 2 + 7, "chunk window");

DmixSpLayout dmix_sp_layout(int M, int C, int T) {
  DmixSpLayout L{};
  L.mix = dmix_layout(M, C, T);
  const size_t mc = (size_t)M * C;
  size_t o = (L.mix.bytes + 15) / 16 * 16;
  L.off_xr = o;   o += (mc * (size_t)T * sizeof(float) + 15) / 16 * 16;
  L.off_plan = o; o += mc * sizeof(DmixEntry);
  L.off_off = o;  o += (mc + 1) * sizeof(int64_t);
  L.bytes = o;
  return L;
}

CTN_DEV int64_t floor_div(int64_t a, int64_t b) {   // b > 0
  const int64_t q = a / b;
  return q * b > a ? q - 1 : q;
}

// First pool sample of the entry's utterance and the utterance's length, or false for an
// entry that must not be read: the T output centres span sp.span input samples from `start`.
CTN_DEV bool sp_entry(const DmixResampleArgs& a, const DmixEntry& e, int32_t k, int64_t* o, int64_t* len) {
  if (k < 0 || k >= a.sp.n || e.utt < 0 || e.utt >= a.U || e.start < 0) return false;
  *o = a.off[e.utt];
  *len = a.off[e.utt + 1] - *o;
  return (int64_t)e.start + a.sp.s[k].span <= *len;
}

// xr[n] = sum_i h[n down - i up + hl] x[i], i upward, acc = fl32(acc + fl32(h x)) from 0
// (include/ctn.h).  grid: (m*C + c) * nchunk + chunk; thread t computes the chunk's outputs
// t, t + 256, ...: neighbouring lanes are neighbouring outputs, whose filter phases
// p = (n down + hl) mod up are distinct (or equal: a broadcast) and whose newest inputs
// q = (n down + hl) / up are at most 2 apart.  With the tap index j = (h index - p) / up the
// same in every lane, the h words of a wave-instruction are p + j up: h in its natural order
// is already the [tap][phase] layout, conflict-free for up <= 32 and 2-way above.
// Input samples outside the utterance are staged as +0 and never read from the pool; adding
// fl32(h * 0) = +-0 to a sum that started at +0 leaves its bits, so this equals skipping them.
template <int DT> __global__ __launch_bounds__(256) void dmix_resample_kernel(DmixResampleArgs a) {
  __shared__ float xw[DMIX_SP_WINDOW];
  __shared__ float hs[DMIX_SP_TAPS + 3];
  const int nchunk = a.L.mix.nchunk;
  const int mc = blockIdx.x / nchunk, chunk = blockIdx.x % nchunk;
  const int tid = threadIdx.x;
  const DmixEntry e = a.plan[mc];
  const int32_t k = a.speed[mc];
  int64_t o = 0, len = 0;
  const bool ok = sp_entry(a, e, k, &o, &len);
  if (chunk == 0 && tid == 0) {   // the tables that present xr to the mix kernels
    reinterpret_cast<DmixEntry*>(a.ws + a.L.off_plan)[mc] = DmixEntry{ok ? mc : -1, 0, e.level_db, e.tries};
    int64_t* off2 = reinterpret_cast<int64_t*>(a.ws + a.L.off_off);
    off2[mc] = (int64_t)mc * a.T;
    if (mc == a.M * a.C - 1) off2[mc + 1] = (int64_t)(mc + 1) * a.T;
  }
  if (!ok) return;                // utt = -1 above: the mix kernels never read this row of xr
  float* xr = reinterpret_cast<float*>(a.ws + a.L.off_xr) + (size_t)mc * a.T;
  const int n0 = chunk * DMIX_CHUNK;
  const int cnt = min(DMIX_CHUNK, a.T - n0);       // outputs of this chunk, >= 1
  const DmixSpeed sp = a.sp.s[k];
  if (sp.up == 1 && sp.down == 1) {                // exact copy
    float x[8];
    load8<DT>(a.pool, o + e.start, n0 + tid * 8, a.T, x);
    store8(xr, n0 + tid * 8, a.T, x);
    return;
  }
  const int up = sp.up, down = sp.down, hl = sp.hl;
  // segment-relative input indices [ilo, ihi] under the chunk's outputs
  const int64_t c0 = (int64_t)n0 * down;
  const int64_t ilo = -floor_div(hl - c0, up);                            // ceil((c0 - hl) / up)
  const int64_t ihi = floor_div(c0 + (int64_t)(cnt - 1) * down + hl, up);
  const int W = (int)(ihi - ilo + 1);                                     // <= DMIX_SP_WINDOW - 7
  for (int t = tid; t <= 2 * hl; t += 256) hs[t] = a.filt[sp.foff + t];
  const int64_t a0 = (int64_t)e.start + ilo;                              // utterance index of xw[0]
  for (int g = tid * 8; g < W; g += 256 * 8) {
    float x[8];
    const int64_t u = a0 + g;
    if (u >= 0 && u + 8 <= len) {
      load8<DT>(a.pool, o + u, 0, 8, x);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        x[i] = 0.f;
        if (u + i >= 0 && u + i < len) {
          if constexpr (DT == 0) x[i] = (float)reinterpret_cast<const int16_t*>(a.pool)[o + u + i] * 0x1p-15f;
          else x[i] = reinterpret_cast<const float*>(a.pool)[o + u + i];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) xw[g + i] = x[i];
  }
  __syncthreads();
  // output n0 + r: t = c0 + hl + r down = q up + p
  const int64_t t0 = c0 + hl;
  const int64_t q0 = t0 / up;
  const int p0 = (int)(t0 - q0 * up);
  const int jfull = 2 * hl / up;
  const unsigned tr = (unsigned)(p0 + tid * down);
  int p = (int)(tr % (unsigned)up);
  int qi = (int)(q0 - ilo) + (int)(tr / (unsigned)up);                    // q - ilo: index into xw
  const int dq = 256 * down / up, dp = 256 * down % up;
  for (int r = tid; r < cnt; r += 256) {
    float acc = 0.f;
    if (p + jfull * up <= 2 * hl) acc = acc + hs[p + jfull * up] * xw[qi - jfull];   // only this tap can be absent
    for (int j = jfull - 1; j >= 0; --j) acc = acc + hs[p + j * up] * xw[qi - j];
    xr[n0 + r] = acc;
    p += dp;
    qi += dq;
    if (p >= up) {
      p -= up;
      qi += 1;
    }
  }
}

hipError_t launch_dmix_resample(const DmixResampleArgs& r, DmixMixArgs* mix, hipStream_t s) {
  const unsigned segs = (unsigned)((long)r.M * r.C * r.L.mix.nchunk);
  if (r.pool_dtype == 0) dmix_resample_kernel<0><<<dim3(segs), dim3(256), 0, s>>>(r);
  else dmix_resample_kernel<1><<<dim3(segs), dim3(256), 0, s>>>(r);
  mix->U = r.M * r.C;
  mix->pool_dtype = 1;
  mix->pool = r.ws + r.L.off_xr;
  mix->off = reinterpret_cast<const int64_t*>(r.ws + r.L.off_off);
  mix->plan = reinterpret_cast<const DmixEntry*>(r.ws + r.L.off_plan);
  mix->ws = r.ws;
  mix->L = r.L.mix;
  return hipGetLastError();
}

hipError_t launch_dmix_mix_sp(const DmixResampleArgs& r, DmixMixArgs mix, hipStream_t s) {
  if (hipError_t e = launch_dmix_resample(r, &mix, s); e != hipSuccess) return e;
  return launch_dmix_mix(mix, s);
}

}  // namespace ctn
