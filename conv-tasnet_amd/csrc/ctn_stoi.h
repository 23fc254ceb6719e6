// STOI / ESTOI on the device: argument block and workspace layout of ctn_stoi.hip
// (include/ctn.h: ctn_stoi_eval).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ctn {

constexpr int STOI_MAX_M = 65535;       // utterances / scored signals per call (one grid dimension)
constexpr int STOI_MAX_C = 16;
constexpr int STOI_MAX_RATIO = 64;      // largest up or down
constexpr int STOI_MAX_HL = 4096;       // largest half length of the resampling filter
constexpr int STOI_FRAME = 256, STOI_HOP = 128, STOI_NFFT = 512, STOI_BANDS = 15, STOI_SEG = 30;
constexpr int STOI_CHUNK = 256;         // frames per step of the compaction's prefix sum
constexpr int STOI_SEG_PER_WAVE = 4;    // segments of a pair per wave of the segment kernel (60 of 64 lanes)
constexpr int STOI_TAB_FILTER = STOI_FRAME + STOI_NFFT;   // offset of the filter in the table

// Offsets in bytes into the caller's workspace.
struct StoiLayout {
  long n10max;         // resampled samples per row, ceil(T up / down)
  int Kmax;            // frames per row, (n10max - 256) / 128 + 1 (0 below 256 samples)
  int Jmax;            // segments per pair, Kmax - 29 (0 below 30 frames)
  size_t off_ref;      // double [M * C][n10max]  resampled references
  size_t off_sig;      // double [M * E][n10max]  resampled signals
  size_t off_nrm;      // double [M * C][Kmax]    2-norms of the references' windowed frames
  size_t off_idx;      // int32  [M * C][Kmax]    numbers of the kept frames
  size_t off_xy;       // double [M * E * C][Kmax][2][15]  band envelopes X, Y
  size_t off_part;     // double [M * E * C][Jmax][2]      STOI / ESTOI sums of a segment
  size_t bytes;
};

struct StoiArgs {
  int M, C, E, T, up, down, Hl;
  const float* refs;        // [M][C][T]
  const float* sigs;        // [M][E][T]
  const int32_t* lengths;   // [M]
  const double* tab;        // window, twiddles, filter
  double* score;            // [M][E][C][2]
  int32_t* kept;            // [M][C]
  int32_t* status;          // [M][C]
  char* ws;
  StoiLayout L;
};

StoiLayout stoi_layout(int M, int C, int E, int T, int up, int down);
hipError_t launch_stoi_eval(const StoiArgs& a, hipStream_t s);

}  // namespace ctn
