// Dynamic mixing with reverberation and noise: argument blocks and workspace layout of
// ctn_dmix_aug.hip (include/ctn.h: ctn_dmix_draw_aug, ctn_dmix_mix_aug).
#pragma once
#include "ctn_dmix.h"

namespace ctn {

constexpr int DMIX_MAX_RIR_TAPS = 16384;   // longest room impulse response
constexpr int DMIX_RIR_TILE = 512;         // taps staged in LDS at a time
constexpr int DMIX_RIR_OUT = 8;            // consecutive outputs per thread: 256 x 8 = DMIX_CHUNK

struct DmixAugDrawArgs {
  int M, C, T;
  uint32_t seed_lo, seed_hi;
  int64_t first;
  const int64_t* first_dev;   // read before launch_dmix_draw advances it
  int32_t n_rirs;             // 0: rir (when given) is all -1
  float rir_prob;
  int32_t* rir;               // [M][C] or null
  int32_t NU, NE;             // noise utterances, eligible entries; NU == 0: no noise plan
  const int64_t* noff;        // [NU+1]
  const int32_t* nelig;       // [NE]
  float snr_lo, snr_hi;
  DmixEntry* nplan;           // [M] or null
};

// Byte offsets into the caller's workspace: the speed-perturbation layout first (the plain mix's
// own workspace when there is no speed table), then the reverberated segments with the tables
// that present them to the mix kernels as an fp32 pool, then the noise stage's partial sums.
struct DmixAugLayout {
  DmixSpLayout sp;     // sp.bytes == sp.mix.bytes without a speed table
  size_t off_xv;       // float [M*C][T]
  size_t off_vplan;    // DmixEntry [M*C]
  size_t off_voff;     // int64 [M*C + 1]
  size_t off_pw;       // double [M][nchunk][2]: per-chunk sums of s^2 and z^2
  size_t off_ng0;      // float [M]: the noise gain before the guard
  size_t bytes;
};

struct DmixReverbArgs {
  int M, C, T, U, pool_dtype;   // the source view: the corpus, or the resampled pool
  const void* pool;
  const int64_t* off;
  const DmixEntry* plan;
  int32_t n_rirs, max_taps;
  const float* rir_pool;
  const int64_t* roff;          // [n_rirs+1]
  const int32_t* rir;           // [M][C]
  char* ws;
  DmixAugLayout L;
};

struct DmixNoiseArgs {
  int NU, dtype;
  const void* pool;
  const int64_t* off;           // [NU+1]
  const DmixEntry* nplan;       // [M]
  float* ngain;                 // [M]
  float* noise_out;             // [M][T] or null
  size_t off_pw, off_ng0;       // into DmixMixArgs::ws
};

DmixAugLayout dmix_aug_layout(int M, int C, int T, bool speeds, bool rirs, bool noise);
hipError_t launch_dmix_draw_aug(const DmixAugDrawArgs& a, hipStream_t s);
// Writes xv and its tables and points `mix` at them.
hipError_t launch_dmix_reverb(const DmixReverbArgs& r, DmixMixArgs* mix, hipStream_t s);
// The level, noise, peak-guard and write stages on the view `mix` with one noise segment per row.
hipError_t launch_dmix_mix_noise(const DmixMixArgs& mix, const DmixNoiseArgs& n, hipStream_t s);

}  // namespace ctn
