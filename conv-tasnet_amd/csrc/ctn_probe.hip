// Hardware probes behind bench.py's measured ceilings (gfx950): the streaming copy
// (ctn_copy_bytes) and the MFMA throughput microbenchmark (ctn_mfma_peak).  Not part of
// any training or inference step.
#include "ctn_common.h"
#include "ctn_kernels.h"

namespace ctn {

// Streaming copy (bench.py's measured bandwidth ceiling, ctn_copy_bytes): 16 B per lane,
// U independent loads in flight per lane before their stores, grid-stride; NT: the loads
// and stores carry the nontemporal hint.
template <int U, bool NT>
__global__ __launch_bounds__(256) void copy_stream_kernel(const v4u* __restrict__ src, v4u* __restrict__ dst,
                                                          long n16) {
  const long stride = (long)gridDim.x * 256;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  for (; i + (U - 1) * stride < n16; i += U * stride) {
    v4u v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) v[u] = NT ? __builtin_nontemporal_load(src + i + u * stride) : src[i + u * stride];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (NT) __builtin_nontemporal_store(v[u], dst + i + u * stride);
      else dst[i + u * stride] = v[u];
    }
  }
  for (; i < n16; i += stride) dst[i] = src[i];
}

hipError_t launch_copy_stream(void* dst, const void* src, size_t bytes, int wgs, int flags, hipStream_t s) {
  if (!dst || !src || bytes % 16 || ((uintptr_t)dst | (uintptr_t)src) % 16 || wgs < 1 || wgs > 65536 ||
      (flags & ~3))
    return hipErrorInvalidValue;
  if (!bytes) return hipSuccess;
  const v4u* a = (const v4u*)src;
  v4u* b = (v4u*)dst;
  const long n = (long)(bytes / 16);
  switch (flags) {
    case 0: hipLaunchKernelGGL((copy_stream_kernel<4, false>), dim3(wgs), dim3(256), 0, s, a, b, n); break;
    case 1: hipLaunchKernelGGL((copy_stream_kernel<4, true>), dim3(wgs), dim3(256), 0, s, a, b, n); break;
    case 2: hipLaunchKernelGGL((copy_stream_kernel<8, false>), dim3(wgs), dim3(256), 0, s, a, b, n); break;
    default: hipLaunchKernelGGL((copy_stream_kernel<8, true>), dim3(wgs), dim3(256), 0, s, a, b, n); break;
  }
  return hipGetLastError();
}

// MFMA throughput microbenchmark (bench.py's measured matrix peak beside the 2.5 PF/s
// datasheet value, ctn_mfma_peak): every wave issues `iters` rounds of NACC independent
// back-to-back bf16 MFMAs on register operands drawn from a hash of its lane (random
// data: the chip holds a lower clock on random than on zero operands), and writes its
// accumulators so nothing is dead.  SHAPE 0: v_mfma_f32_16x16x32_bf16 (16384 FLOP, the
// block kernels' instruction), 1: v_mfma_f32_32x32x16_bf16 (32768 FLOP).
typedef short mp_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mp_f32x4 __attribute__((ext_vector_type(4)));
typedef float mp_f32x16 __attribute__((ext_vector_type(16)));
template <int SHAPE>
__global__ __launch_bounds__(256) void mfma_peak_kernel(int iters, float* out) {
  constexpr int NACC = SHAPE == 0 ? 8 : 4;
  const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
  uint32_t h = gid * 2654435761u + 12345u;
  short av[8], bv[8];
  for (int e = 0; e < 8; ++e) {
    h ^= h << 13; h ^= h >> 17; h ^= h << 5;
    av[e] = (short)(0x3800 | (h & 0x807f));   // bf16 of magnitude ~2^-15..2^-14, random sign and mantissa
    h ^= h << 13; h ^= h >> 17; h ^= h << 5;
    bv[e] = (short)(0x3800 | (h & 0x807f));
  }
  const mp_bf16x8 a = {av[0], av[1], av[2], av[3], av[4], av[5], av[6], av[7]};
  const mp_bf16x8 b = {bv[0], bv[1], bv[2], bv[3], bv[4], bv[5], bv[6], bv[7]};
  float sum = 0.f;
  if constexpr (SHAPE == 0) {
    mp_f32x4 acc[NACC];
    for (int j = 0; j < NACC; ++j) acc[j] = mp_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j], 0, 0, 0);
    for (int j = 0; j < NACC; ++j) sum += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  } else {
    mp_f32x16 acc[NACC];
    for (int j = 0; j < NACC; ++j)
      for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    for (int it = 0; it < iters; ++it)
#pragma unroll
      for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
    for (int j = 0; j < NACC; ++j)
      for (int e = 0; e < 16; ++e) sum += acc[j][e];
  }
  out[gid] = sum;
}

hipError_t launch_mfma_peak(int shape, int wgs, int iters, float* out, double* flops, hipStream_t s) {
  if (!out || wgs < 1 || wgs > 65536 || iters < 1 || (shape != 0 && shape != 1)) return hipErrorInvalidValue;
  // waves x iterations x independent accumulators x FLOP per instruction
  if (flops) *flops = (double)wgs * 4 * iters * (shape == 0 ? 8.0 * 16384 : 4.0 * 32768);
  if (shape == 0) hipLaunchKernelGGL((mfma_peak_kernel<0>), dim3(wgs), dim3(256), 0, s, iters, out);
  else hipLaunchKernelGGL((mfma_peak_kernel<1>), dim3(wgs), dim3(256), 0, s, iters, out);
  return hipGetLastError();
}

}  // namespace ctn
