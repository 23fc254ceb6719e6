// Windowed separation: argument block and launchers of ctn_stitch.hip (include/ctn.h
// ctn_stitch_*).
#pragma once
#include "ctn_common.h"

namespace ctn {

constexpr int STITCH_MIN_C = 2, STITCH_MAX_C = 8;   // the search is over all C! permutations
constexpr int STITCH_THREADS = 256;
constexpr int STITCH_CHUNK = 2048;   // overlap samples per correlation workgroup: 256 threads x 2 x 4

struct StitchArgs {
  int J, C, W, O, T, Hs;
  int nchunk;               // ceil(O / STITCH_CHUNK)
  bool vec;                 // W and O multiples of 4 and every pointer 16-byte aligned
  bool vec_out;             // ola: T a multiple of 4 too, rows of `out` stay aligned
  const float* x;           // [T]
  float* win;               // [J][W]
  const float* P;           // [J][C][W]
  double* part;             // workspace [(J-1)][nchunk][C][C]
  double* sim;              // [J][C][C]
  int32_t* perm;            // [J][C]
  int32_t* sigma;           // [J][C]
  int32_t* status;          // [J]
  const int32_t* sigma_in;  // ola
  const float* fade;        // [O]
  float* out;               // [C][T]
};

inline int stitch_window_count(long T, long W, long Hs) { return T <= W ? 1 : (int)(1 + (T - W + Hs - 1) / Hs); }
inline int stitch_nchunk(int O) { return (O + STITCH_CHUNK - 1) / STITCH_CHUNK; }

hipError_t launch_stitch_frame(const StitchArgs& a, hipStream_t s);
// correlation partials, then sums + permutation search, then the chain scan
hipError_t launch_stitch_plan(const StitchArgs& a, hipStream_t s);
hipError_t launch_stitch_ola(const StitchArgs& a, hipStream_t s);

}  // namespace ctn
