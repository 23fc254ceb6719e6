// Reduction plumbing shared by all kernels (gfx950): the statistics finalize launches
// (slab partials -> (mean, rstd) or (S / cnt, SS / cnt)), the fixed-order slab reduce of
// the parameter-gradient partials, and the fp32 -> storage-type weight preparation.
#include <vector>

#include "ctn_common.h"
#include "ctn_kernels.h"

namespace ctn {

// ===========================================================================
// statistics finalize / slab reduce / weight prep
// ===========================================================================
// one thread per group (few parts, e.g. cLN rows) ...
__global__ __launch_bounds__(256) void stats_finalize_thread_kernel(const double2* slab, int G, int nparts, double cnt,
                                                                    int mode, float eps, float2* out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= G) return;
  double s = 0.0, ss = 0.0;
  for (int i = 0; i < nparts; ++i) {
    const double2 v = slab[(size_t)g * nparts + i];
    s += v.x;
    ss += v.y;
  }
  out[g] = stat_finish(mode, s, ss, cnt, eps);
}

// ... or a tile of 64 groups per workgroup staged through LDS with coalesced loads
// (cLN: 516k rows x 16 parts at c4; a thread walking its own row's parts read the
// slab with a 256-byte lane stride), summed per thread in the same part order
constexpr int SF_ROWS = 64;
__global__ __launch_bounds__(256) void stats_finalize_tile_kernel(const double2* slab, int G, int nparts, double cnt,
                                                                  int mode, float eps, float2* out) {
  extern __shared__ double2 sh[];   // [SF_ROWS][nparts + 1] (padded row: 4-way banks)
  const long g0 = (long)blockIdx.x * SF_ROWS;
  const int rows = (int)(G - g0 < SF_ROWS ? G - g0 : SF_ROWS);
  const int n = rows * nparts;
  for (int i = threadIdx.x; i < n; i += 256) sh[(i / nparts) * (nparts + 1) + i % nparts] = slab[g0 * nparts + i];
  __syncthreads();
  if (threadIdx.x >= rows) return;
  double s = 0.0, ss = 0.0;
  for (int i = 0; i < nparts; ++i) {
    const double2 v = sh[threadIdx.x * (nparts + 1) + i];
    s += v.x;
    ss += v.y;
  }
  const long g = g0 + threadIdx.x;
  out[g] = stat_finish(mode, s, ss, cnt, eps);
}

// ... or one workgroup per group (many parts, e.g. gLN utterances)
__global__ __launch_bounds__(256) void stats_finalize_block_kernel(const double2* slab, int nparts, double cnt,
                                                                   int mode, float eps, float2* out) {
  __shared__ double red[8];
  const int g = blockIdx.x;
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < nparts; i += 256) {
    const double2 x = slab[(size_t)g * nparts + i];
    v[0] += x.x;
    v[1] += x.y;
  }
  block_sum_d<2>(v, red);
  if (threadIdx.x == 0) out[g] = stat_finish(mode, v[0], v[1], cnt, eps);
}

hipError_t launch_stats_finalize(const double2* slab, int G, int nparts, double cnt, int mode, float eps,
                                 float2* out, hipStream_t s) {
  // one workgroup per group only when groups are few and long (gLN: one per
  // utterance); cLN has a group per frame row (G = M*Kp, 516k at c4), where a
  // workgroup per row cost 540 us per launch against a few us for a thread per row
  if (nparts >= 8 && (G < 8192 || nparts > 64))
    hipLaunchKernelGGL(stats_finalize_block_kernel, dim3(G), dim3(256), 0, s, slab, nparts, cnt, mode, eps, out);
  else if (nparts >= 2)
    hipLaunchKernelGGL(stats_finalize_tile_kernel, dim3((G + SF_ROWS - 1) / SF_ROWS), dim3(256),
                       (size_t)SF_ROWS * (nparts + 1) * sizeof(double2), s, slab, G, nparts, cnt, mode, eps, out);
  else
    hipLaunchKernelGGL(stats_finalize_thread_kernel, dim3((G + 255) / 256), dim3(256), 0, s, slab, G, nparts, cnt,
                       mode, eps, out);
  return hipGetLastError();
}

// out[i] = sum_q src[q * pstride + i], deterministic, fp64 accumulation.
// Workgroup = one 64-output tile x one slice of <= SR_SLICE parts of one
// descriptor; wave w sums parts w, w+4, ... of the slice (lanes = 64
// consecutive outputs: 256-byte rows, loads unrolled 8 deep); the 4 wave
// partials combine in a fixed order.  Descriptors with more than one slice
// write slice partials to `tmp` and a second pass sums the slices in order.
constexpr int SR_SLICE = 64;

struct SrJob {
  const float* src;
  float* dst;
  int nparts, n, pstride, nslices;
  int vec4;   // 4 consecutive outputs per lane (16-byte loads); same per-output order
};
// The grid is flat: job jb owns workgroups [wg0[jb], wg0[jb+1]), one per (slice, output
// tile) pair, so no workgroup is launched only to exit (a (tiles, slices, jobs) grid sized
// by the largest job launched ~70k workgroups per block backward for ~1.3k with work).
// Up to SR_MAXJ jobs per launch (kernel arguments: ~3 KiB): a whole backward's deferred
// reductions (ctn_tblock_reduce_grads) take a few launches instead of two per block.
constexpr int SR_MAXJ = 64;
struct SrBatch {
  SrJob j[SR_MAXJ];
  int wg0[SR_MAXJ + 1];   // prefix sums of the jobs' workgroup counts
  int ntx[SR_MAXJ];       // output tiles per slice
  int nj;
};

__global__ __launch_bounds__(256) void slab_reduce_kernel(SrBatch b) {
  __shared__ double part[4][64];
  __shared__ double part4[4][4][64];
  int jb = 0;   // the job owning this workgroup: binary search of the prefix sums
  for (int step = SR_MAXJ / 2; step > 0; step >>= 1)
    if (jb + step < b.nj && (int)blockIdx.x >= b.wg0[jb + step]) jb += step;
  const SrJob d = b.j[jb];
  const int ntx = b.ntx[jb];
  const int loc = (int)blockIdx.x - b.wg0[jb];
  const int sl = loc / ntx, tx = loc - sl * ntx;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int q0 = sl * SR_SLICE;
  const int q1 = d.nslices == 1 ? d.nparts : (q0 + SR_SLICE < d.nparts ? q0 + SR_SLICE : d.nparts);
  float* out = d.nslices > 1 ? d.dst + (size_t)sl * d.n : d.dst;
  if (d.vec4) {   // lanes own 4 consecutive outputs: 1 KiB per wave load instead of 256 B
    for (int i0 = tx * 256; i0 < d.n; i0 += ntx * 256) {
      const int i = i0 + 4 * lane;
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
      if (i < d.n) {
        const float* src = d.src + i;
        int q = q0 + w;
        for (; q + 28 < q1; q += 32) {
          float4 v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(src + (size_t)(q + 4 * u) * d.pstride);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            a0 += (double)v[u].x;
            a1 += (double)v[u].y;
            a2 += (double)v[u].z;
            a3 += (double)v[u].w;
          }
        }
        for (; q < q1; q += 4) {
          const float4 v = *reinterpret_cast<const float4*>(src + (size_t)q * d.pstride);
          a0 += (double)v.x;
          a1 += (double)v.y;
          a2 += (double)v.z;
          a3 += (double)v.w;
        }
      }
      part4[w][0][lane] = a0;
      part4[w][1][lane] = a1;
      part4[w][2][lane] = a2;
      part4[w][3][lane] = a3;
      __syncthreads();
      if (w == 0 && i < d.n) {
        float4 o;
        o.x = (float)(((part4[0][0][lane] + part4[1][0][lane]) + part4[2][0][lane]) + part4[3][0][lane]);
        o.y = (float)(((part4[0][1][lane] + part4[1][1][lane]) + part4[2][1][lane]) + part4[3][1][lane]);
        o.z = (float)(((part4[0][2][lane] + part4[1][2][lane]) + part4[2][2][lane]) + part4[3][2][lane]);
        o.w = (float)(((part4[0][3][lane] + part4[1][3][lane]) + part4[2][3][lane]) + part4[3][3][lane]);
        *reinterpret_cast<float4*>(out + i) = o;
      }
      __syncthreads();
    }
    return;
  }
  for (int i0 = tx * 64; i0 < d.n; i0 += ntx * 64) {
    const int i = i0 + lane;
    double acc = 0.0;
    if (i < d.n) {
      const float* src = d.src + i;
      int q = q0 + w;
      for (; q + 28 < q1; q += 32) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(q + 4 * u) * d.pstride];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += (double)v[u];
      }
      for (; q < q1; q += 4) acc += (double)src[(size_t)q * d.pstride];
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && i < d.n) out[i] = (float)(((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
    __syncthreads();
  }
}

static hipError_t sr_launch(SrBatch b, hipStream_t s) {
  if (b.nj <= 0) return hipSuccess;
  long tot = 0;
  for (int i = 0; i < b.nj; ++i) {
    const int per = b.j[i].vec4 ? 256 : 64;
    int g = (b.j[i].n + per - 1) / per;
    if (g > 1024) g = 1024;   // larger outputs: grid-stride over the tiles
    if (g < 1) g = 1;
    b.ntx[i] = g;
    b.wg0[i] = (int)tot;
    tot += (long)g * b.j[i].nslices;
  }
  b.wg0[b.nj] = (int)tot;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)tot), dim3(256), 0, s, b);
  return hipGetLastError();
}

size_t slab_reduce_tmp_floats(const SlabBatch& b) {
  size_t t = 0;
  for (int i = 0; i < b.nd; ++i) {
    const int ns = (b.d[i].nparts + SR_SLICE - 1) / SR_SLICE;
    if (ns > 1) t += (size_t)ns * b.d[i].n;
  }
  return t;
}

// Scratch of each descriptor with more than one slice, carved from `tmp` in descriptor
// order (slab_reduce_tmp_floats' sizing); null where one pass suffices or tmp is null.
void slab_reduce_assign_tmp(const SlabDesc* d, int n, float* tmp, float** out) {
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const int ns = (d[i].nparts + SR_SLICE - 1) / SR_SLICE;
    out[i] = nullptr;
    if (ns > 1 && tmp) {
      out[i] = tmp + off;
      off += (size_t)ns * d[i].n;
    }
  }
}

// Every first pass (slice partials) of the list, then every second pass, SR_MAXJ jobs per
// launch.  Each descriptor's per-output summation order is that of launch_slab_reduce.
hipError_t launch_slab_reduce_list(const SlabDesc* descs, float* const* tmps, int n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  std::vector<SrJob> j1, j2;
  auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  for (int i = 0; i < n; ++i) {
    const SlabDesc& d = descs[i];
    const int ns = (d.nparts + SR_SLICE - 1) / SR_SLICE;
    const bool v4 = d.n % 4 == 0 && d.pstride % 4 == 0 && a16(d.src) && a16(d.dst);
    float* t = tmps ? tmps[i] : nullptr;
    if (ns <= 1 || !t) {
      // single pass straight into dst (also the fallback when no scratch is given)
      j2.push_back(SrJob{d.src, d.dst, d.nparts, d.n, d.pstride, 1, v4 ? 1 : 0});
    } else {
      const bool v4t = v4 && a16(t);
      j1.push_back(SrJob{d.src, t, d.nparts, d.n, d.pstride, ns, v4t ? 1 : 0});
      j2.push_back(SrJob{t, d.dst, ns, d.n, d.n, 1, v4t ? 1 : 0});
    }
  }
  for (const std::vector<SrJob>* js : {&j1, &j2}) {
    for (size_t k = 0; k < js->size(); k += SR_MAXJ) {
      SrBatch b{};
      for (size_t i = k; i < js->size() && b.nj < SR_MAXJ; ++i) b.j[b.nj++] = (*js)[i];
      const hipError_t e = sr_launch(b, s);
      if (e != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

hipError_t launch_slab_reduce(const SlabBatch& b, float* tmp, hipStream_t s) {
  float* tmps[12];
  slab_reduce_assign_tmp(b.d, b.nd, tmp, tmps);
  return launch_slab_reduce_list(b.d, tmps, b.nd, s);
}

// fp32 [O][I] weight -> storage-type copy Ws [O][I] and/or transpose Wt [I][O], one
// 64x64 tile per workgroup through LDS: both the row-major reads/writes and the
// transposed writes are coalesced.  grid = (tiles of the largest matrix, nd).
constexpr int PW_T = 64;
template <typename T>
__global__ __launch_bounds__(256) void prep_weight_kernel(PrepBatch pb) {
  __shared__ float tile[PW_T][PW_T + 1];
  const PrepDesc d = pb.d[blockIdx.y];
  const int tcol = (d.I + PW_T - 1) / PW_T, trow = (d.O + PW_T - 1) / PW_T;
  if ((int)blockIdx.x >= tcol * trow) return;
  const int r0 = (blockIdx.x / tcol) * PW_T, c0 = (blockIdx.x % tcol) * PW_T;
  T* Ws = reinterpret_cast<T*>(d.Ws);
  T* Wt = reinterpret_cast<T*>(d.Wt);
  for (int i = threadIdx.x; i < PW_T * PW_T; i += 256) {
    const int r = i / PW_T, c = i % PW_T;
    float v = 0.f;
    if (r0 + r < d.O && c0 + c < d.I) {
      v = d.W[(size_t)(r0 + r) * d.I + c0 + c];
      if (Ws) st1<T>(Ws + (size_t)(r0 + r) * d.I + c0 + c, v);
    }
    tile[r][c] = v;
  }
  if (!Wt && !d.Wf && !d.Wtf) return;
  __syncthreads();
  if (Wt) {
    for (int i = threadIdx.x; i < PW_T * PW_T; i += 256) {
      const int c = i / PW_T, r = i % PW_T;
      if (r0 + r < d.O && c0 + c < d.I) st1<T>(Wt + (size_t)(c0 + c) * d.O + r0 + r, tile[r][c]);
    }
  }
  // fragment-order copies (frag_offset; O and I are multiples of 32, checked by the
  // caller, so the tile holds whole 32x32 fragment pairs): 512 pieces of 8 per copy
  for (int pass = 0; pass < 2; ++pass) {
    T* F = reinterpret_cast<T*>(pass ? d.Wtf : d.Wf);
    if (!F) continue;
    const int Icols = pass ? d.O : d.I;     // reduction length of the copy
    const int gb = (pass ? c0 : r0) / 32, kb0 = (pass ? r0 : c0) / 32;
    for (int i = threadIdx.x; i < 512; i += 256) {
      const int lane = i & 63, nb = (i >> 6) & 1, kb = (i >> 7) & 1, g = i >> 8;
      const int n = g * 32 + ((lane & 15) >> 2) * 8 + nb * 4 + (lane & 3), k = kb * 32 + (lane >> 4) * 8;
      if ((pass ? c0 + n >= d.I || r0 + k >= d.O : r0 + n >= d.O || c0 + k >= d.I)) continue;
      T* dst = F + frag_offset(gb + g, nb, kb0 + kb, lane, Icols);
#pragma unroll
      for (int e = 0; e < 8; ++e) st1<T>(dst + e, pass ? tile[k + e][n] : tile[n][k + e]);
    }
  }
}

hipError_t launch_prep_weights(DType dt, const PrepBatch& pb, hipStream_t s) {
  if (pb.nd <= 0) return hipSuccess;
  if (pb.nd > PREP_MAX) return hipErrorInvalidValue;
  int mx = 1;
  for (int i = 0; i < pb.nd; ++i) {
    const int t = ((pb.d[i].O + PW_T - 1) / PW_T) * ((pb.d[i].I + PW_T - 1) / PW_T);
    mx = t > mx ? t : mx;
  }
  if (dt == BF16) hipLaunchKernelGGL(prep_weight_kernel<bf16raw>, dim3(mx, pb.nd), dim3(256), 0, s, pb);
  else hipLaunchKernelGGL(prep_weight_kernel<float>, dim3(mx, pb.nd), dim3(256), 0, s, pb);
  return hipGetLastError();
}

hipError_t launch_prep_weight(DType dt, const float* W, int O, int I, void* Ws, void* Wt, hipStream_t s) {
  PrepBatch pb{};
  pb.d[0] = PrepDesc{W, O, I, Ws, Wt, nullptr, nullptr};
  pb.nd = 1;
  return launch_prep_weights(dt, pb, s);
}

}  // namespace ctn
