// Internal launcher interface for the PIT loss with silent sources (ctn_pitvar.hip).
#pragma once
#include "ctn_kernels.h"

namespace ctn {

constexpr int PITVAR_CMIN = 2, PITVAR_CMAX = 8;

struct PitVarArgs {
  int M, C, T;
  int mode;                      // 0 thresholded SNR, 1 SI-SNR (active references)
  double tau, tau0;              // 10^(-snr_max/10), 10^(-inactive_snr_max/10)
  const float* src;              // [M][C][T] references
  const float* est;              // [M][C][T]
  const float* mix;              // [M][T] or null: x = sum_j s_j
  const int64_t* lengths;        // [M]
  double* slab;                  // [M][chunks][NV]
  int chunks;
  double* msd;                   // [M] max_snr in fp64 (pitvar_final -> pitvar_loss)
  float* max_snr;                // [M]
  int64_t* perm;                 // [M][C] reference of output i
  uint8_t* active;               // [M][C] 1: reference j has a non-zero sample inside the length
  float* coef;                   // [M][C][4]: al, be, off, j
  float* loss;                   // [1]
  const float* g_loss;           // upstream dL/d loss [1] (backward)
  const float* g_maxsnr;         // upstream dL/d max_snr [M] or null (backward)
  float* gest;                   // [M][C][T] (backward)
};
int pitvar_nv(int C);            // statistics per (utterance, chunk)
hipError_t launch_pitvar_forward(const PitVarArgs& a, hipStream_t s);
hipError_t launch_pitvar_backward(const PitVarArgs& a, hipStream_t s);

}  // namespace ctn
