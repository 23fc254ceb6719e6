// Internal launcher interface for the MixIT loss kernels (ctn_mixit.hip).
#pragma once
#include "ctn_kernels.h"

namespace ctn {

constexpr int MIXIT_CMIN = 2, MIXIT_CMAX = 8;

struct MixitArgs {
  int M, C, T;
  int mode;                      // 0 thresholded SNR, 1 SI-SNR
  double tau;                    // 10^(-snr_max/10) (mode 0)
  const float* mix;              // [M][2][T] the two recordings
  const float* est;              // [M][C][T]
  const int64_t* lengths;        // [M]
  double* slab;                  // [M][chunks][NV]
  int chunks;
  double* msd;                   // [M] max_snr in fp64 (mixit_search -> mixit_loss)
  float* max_snr;                // [M]
  int64_t* assign;               // [M] winning assignment, bit c = recording of output c
  float* coef;                   // [M][2][4]: al, be, off, unused
  float* loss;                   // [1]
  float* remix;                  // [M][2][T] or null
  const float* g_loss;           // upstream dL/d loss [1] (backward)
  const float* g_maxsnr;         // upstream dL/d max_snr [M] or null (backward)
  float* gest;                   // [M][C][T] (backward)
};
int mixit_nv(int C);             // statistics per (utterance, chunk)
hipError_t launch_mixit_forward(const MixitArgs& a, hipStream_t s);
hipError_t launch_mixit_backward(const MixitArgs& a, hipStream_t s);

}  // namespace ctn
