// Internal launcher interface for the mixture-consistency kernels (ctn_mixcon.hip).
#pragma once
#include "ctn_kernels.h"

namespace ctn {

constexpr int MIXCON_CMIN = 2, MIXCON_CMAX = 16;
constexpr int MIXCON_UNIFORM = 0, MIXCON_POWER = 1;

struct MixconArgs {
  int M, C, T;
  int mode;                      // MIXCON_UNIFORM / MIXCON_POWER
  const float* x;                // [M][T] the mixture
  const float* s;                // [M][C][T] the model's outputs
  const int64_t* lengths;        // [M] or null (= T)
  int chunks;                    // T-chunks of the statistics passes
  double* slab;                  // [M][chunks][C] chunk partials (power)
  double* coef;                  // [M][C+1]: w_c, D (power; written by the forward)
  double* kcoef;                 // [M][C]: 2 (a_c - sum_j w_j a_j) / D (power, backward)
  float* y;                      // [M][C][T] (forward)
  const float* g;                // [M][C][T] upstream dL/dy (backward)
  float* gs;                     // [M][C][T] dL/ds (backward)
  float* gx;                     // [M][T] dL/dx or null (backward)
};
hipError_t launch_mixcon_forward(const MixconArgs& a, hipStream_t s);
hipError_t launch_mixcon_backward(const MixconArgs& a, hipStream_t s);

}  // namespace ctn
