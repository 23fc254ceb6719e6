// BSS Eval v3 (bss_eval_sources) on the device: argument block and workspace layout of
// ctn_bss.hip (include/ctn.h: ctn_bss_eval).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ctn {

constexpr int BSS_MAX_ORDER = 4096;   // largest normal-equation system, C * flen
constexpr int BSS_MAX_M = 65535;      // utterances per call (one grid dimension)

// Offsets (in doubles) into the caller's workspace; every per-utterance slab is contiguous.
struct BssLayout {
  int NP;              // reference pairs i <= j
  int nchunk;          // T chunks of the lag correlations
  int ntile;           // output tiles of the projection
  int nsys;            // systems per utterance: the full one, then C single-reference ones (C > 1)
  size_t LV;           // lag values per utterance: NP * (2 flen - 1) then E * C * flen
  size_t sys_elems;    // Gram matrix doubles per utterance
  size_t coef_elems;   // right-hand sides / coefficients per utterance
  size_t off_part, off_lag, off_gram, off_coef, off_epart, off_flag;
  size_t bytes;
};

struct BssArgs {
  int M, C, E, T, flen;
  const float* refs;        // [M][C][T]
  const float* sigs;        // [M][E][T]
  const int32_t* lengths;   // [M]
  double* energies;         // [M][E][C][5]
  int32_t* status;          // [M]
  double* ws;
  BssLayout L;
};

BssLayout bss_layout(int M, int C, int E, int T, int flen);
hipError_t launch_bss_eval(const BssArgs& a, hipStream_t s);

}  // namespace ctn
