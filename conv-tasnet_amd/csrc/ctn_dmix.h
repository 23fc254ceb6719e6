// Dynamic mixing on the device: argument blocks and workspace layout of ctn_dmix.hip
// (include/ctn.h: ctn_dmix_draw, ctn_dmix_mix).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ctn {

constexpr int DMIX_MAX_C = 16;        // slots per row (the PIT loss's limit)
constexpr int DMIX_MAX_TRIES = 64;    // candidates per slot
constexpr int DMIX_CHUNK = 2048;      // samples per workgroup: 256 threads x 8

struct DmixEntry {                    // == ctn_dmix_entry
  int32_t utt, start;
  float level_db;
  int32_t tries;
};

// Byte offsets into the caller's workspace.
struct DmixLayout {
  int nchunk;          // chunks of DMIX_CHUNK samples per segment
  size_t off_ssq;      // double [M*C][nchunk]: per-chunk sums of squares (level_mode 1)
  size_t off_g0;       // float  [M*C]: gains before the peak guard
  size_t off_pmax;     // float  [M][nchunk]: per-chunk peaks of the unguarded mixture
  size_t bytes;
};

struct DmixDrawArgs {
  int M, C, T, U, E, max_tries;
  float lo_db, hi_db;
  uint32_t seed_lo, seed_hi;
  const int64_t* off;         // [U+1]
  const int32_t* spk;         // [U]
  const int32_t* elig;        // [E]
  int64_t first;              // global sample of row 0 when first_dev is null
  int64_t* first_dev;
  int64_t advance;            // added to *first_dev by a second kernel
  DmixEntry* plan;            // [M][C]
};

struct DmixMixArgs {
  int M, C, T, U, pool_dtype, level_mode;
  float peak;
  const void* pool;
  const int64_t* off;         // [U+1]
  const DmixEntry* plan;      // [M][C]
  float* gains;               // [M][C]
  float* sources;             // [M][C][T]
  float* mixture;             // [M][T]
  int32_t* status;            // [M]
  char* ws;
  DmixLayout L;
};

DmixLayout dmix_layout(int M, int C, int T);
hipError_t launch_dmix_draw(const DmixDrawArgs& a, hipStream_t s);
hipError_t launch_dmix_mix(const DmixMixArgs& a, hipStream_t s);

}  // namespace ctn
