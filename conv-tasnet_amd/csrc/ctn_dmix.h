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
constexpr int DMIX_MAX_SPEEDS = 8;    // entries of a speed table (ctn_dmix_draw_sp, ctn_dmix_mix_sp)

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
  int32_t* speed;             // [M][C] speed index of each slot, or null: the plain draw
  int32_t nspeed;             // with `speed`: entries of `span`
  int64_t span[DMIX_MAX_SPEEDS];   // with `speed`: input samples a segment of speed k needs
};

constexpr uint32_t DMIX_COUNT_SLOT = 48;   // Philox counter word 2 of the speaker-count draw

struct DmixThinArgs {
  int M, C, min_speakers;
  uint32_t seed_lo, seed_hi;
  int64_t first;              // global sample of row 0 when first_dev is null
  const int64_t* first_dev;   // the draw's counter, already advanced by `back`
  int64_t back;
  DmixEntry* plan;            // [M][C]
  int32_t* count;             // [M]
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

// Speed perturbation (ctn_dmix_draw_sp, ctn_dmix_mix_sp).
constexpr int DMIX_MAX_RATIO = 64;    // up, down <= 64; up <= 2 down, down <= 2 up
// Input window of one chunk: (DMIX_CHUNK - 1) * down / up + 2 * Hl / up + 2 <= 4094 + 40 + 2
// samples, staged in groups of 8.
constexpr int DMIX_SP_WINDOW = 4160;
constexpr int DMIX_SP_TAPS = 2 * 10 * DMIX_MAX_RATIO + 1;   // 2 Hl + 1 <= 1281

struct DmixSpeed {
  int32_t up, down, hl;   // hl = 10 * max(up, down); the filter has 2 hl + 1 taps
  int32_t foff;           // first tap in the filter table (1/1: no taps)
  int64_t span;           // floor((T - 1) * down / up) + 1: input samples under the T outputs' centres
};

struct DmixSpeedTable {
  int32_t n;
  DmixSpeed s[DMIX_MAX_SPEEDS];
};

// Byte offsets into the caller's workspace of ctn_dmix_mix_sp: the plain mix's own workspace
// first, then the resampled segments and the tables that present them to the mix kernels as an
// fp32 pool of M*C utterances of T samples.
struct DmixSpLayout {
  DmixLayout mix;
  size_t off_xr;       // float [M*C][T]
  size_t off_plan;     // DmixEntry [M*C]: {utt = m*C + c or -1, start = 0, level_db, tries}
  size_t off_off;      // int64 [M*C + 1]: (m*C + c) * T
  size_t bytes;
};

struct DmixResampleArgs {
  int M, C, T, U, pool_dtype;
  DmixSpeedTable sp;
  const float* filt;          // the table's filters, back to back
  const void* pool;
  const int64_t* off;         // [U+1]
  const DmixEntry* plan;      // [M][C]
  const int32_t* speed;       // [M][C]
  char* ws;
  DmixSpLayout L;
};

DmixLayout dmix_layout(int M, int C, int T);
DmixSpLayout dmix_sp_layout(int M, int C, int T);
hipError_t launch_dmix_draw(const DmixDrawArgs& a, hipStream_t s);
hipError_t launch_dmix_thin(const DmixThinArgs& a, hipStream_t s);
hipError_t launch_dmix_mix(const DmixMixArgs& a, hipStream_t s);
// a.plan, a.off, a.pool, a.U, a.pool_dtype of `mix` are replaced by the resampled pool's.
hipError_t launch_dmix_mix_sp(const DmixResampleArgs& r, DmixMixArgs mix, hipStream_t s);
// The stages that ctn_dmix_aug.hip composes: status and the gains before the guard (ssq + gain0),
// and the resampler alone, which points `mix` at the resampled pool as launch_dmix_mix_sp does.
hipError_t launch_dmix_gain0(const DmixMixArgs& a, hipStream_t s);
hipError_t launch_dmix_resample(const DmixResampleArgs& r, DmixMixArgs* mix, hipStream_t s);

}  // namespace ctn
