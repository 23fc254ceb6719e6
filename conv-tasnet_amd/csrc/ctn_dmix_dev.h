// Dynamic mixing on the device: the device helpers that ctn_dmix.hip and ctn_dmix_aug.hip share
// (Philox4x32-10, segment addressing, the 8-sample loads and stores, the row's ordered sum).
// Include after `#pragma clang fp contract(off)`: every product and sum stays a separate operation.
#pragma once
#include "ctn_common.h"
#include "ctn_dmix.h"

namespace ctn {

struct Philox { uint32_t r[4]; };
CTN_DEV Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}

typedef uint32_t v4u_a2 __attribute__((ext_vector_type(4), aligned(2)));
typedef float v4f_a4 __attribute__((ext_vector_type(4), aligned(4)));

// First pool sample of the entry's segment, or -1 for an entry that must not be read.
CTN_DEV int64_t seg_base(const DmixMixArgs& a, const DmixEntry& e) {
  if (e.utt < 0 || e.utt >= a.U || e.start < 0) return -1;
  const int64_t o = a.off[e.utt], len = a.off[e.utt + 1] - o;
  if ((int64_t)e.start + a.T > len) return -1;
  return o + e.start;
}

// Samples [t0, t0 + 8) of the segment at pool sample `base` (exact in fp32); zeros past T.
template <int DT> CTN_DEV void load8(const void* pool, int64_t base, int t0, int T, float x[8]) {
  if (t0 + 8 <= T) {
    if constexpr (DT == 0) {
      const v4u_a2 v = *reinterpret_cast<const v4u_a2*>(reinterpret_cast<const int16_t*>(pool) + base + t0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[2 * i] = (float)(int16_t)(v[i] & 0xffffu) * 0x1p-15f;
        x[2 * i + 1] = (float)(int16_t)(v[i] >> 16) * 0x1p-15f;
      }
    } else {
      const float* p = reinterpret_cast<const float*>(pool) + base + t0;
      const v4f_a4 lo = *reinterpret_cast<const v4f_a4*>(p), hi = *reinterpret_cast<const v4f_a4*>(p + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] = lo[i];
        x[4 + i] = hi[i];
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      x[i] = 0.f;
      if (t0 + i < T) {
        if constexpr (DT == 0) x[i] = (float)reinterpret_cast<const int16_t*>(pool)[base + t0 + i] * 0x1p-15f;
        else x[i] = reinterpret_cast<const float*>(pool)[base + t0 + i];
      }
    }
  }
}

CTN_DEV void store8(float* row, int t0, int T, const float v[8]) {
  if (t0 + 8 <= T) {
    *reinterpret_cast<v4f_a4*>(row + t0) = v4f_a4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<v4f_a4*>(row + t0 + 4) = v4f_a4{v[4], v[5], v[6], v[7]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (t0 + i < T) row[t0 + i] = v[i];
  }
}

// Block-wide fp32 max (a max has no rounding: any order gives the same bits); valid in thread 0.
CTN_DEV float block_max(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) v = fmaxf(v, red[w]);
  return v;
}

// The row's unguarded mixture samples [t0, t0 + 8): the arithmetic of the final write.
template <int DT> CTN_DEV void mix8(const DmixMixArgs& a, const int64_t* base, const float* g, int t0, float acc[8],
                                    float* sources_row0) {
  for (int c = 0; c < a.C; ++c) {
    float x[8], v[8];
    load8<DT>(a.pool, base[c], t0, a.T, x);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = g[c] * x[i];
      acc[i] = c == 0 ? v[i] : acc[i] + v[i];
    }
    if (sources_row0) store8(sources_row0 + (size_t)c * a.T, t0, a.T, v);
  }
}

}  // namespace ctn
