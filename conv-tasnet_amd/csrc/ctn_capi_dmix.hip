// C-ABI entries of dynamic mixing (include/ctn.h ctn_dmix_*).
#include "ctn_capi_util.h"
#include "ctn_dmix.h"

using namespace ctn;

// ===========================================================================
// Dynamic mixing (draw + mix), ctn_dmix.hip
// ===========================================================================
static_assert(sizeof(ctn_dmix_entry) == sizeof(DmixEntry), "plan entry layout");
static_assert(sizeof(ctn_dmix_desc) == 56, "ctn_dmix_desc layout");

static int dmix_check(const ctn_dmix_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->T < 1 || d->n_utts < 1 || d->n_elig < 1)
    return fail(CTN_ERR_ARG, "bad dynamic-mix descriptor M=%d T=%d n_utts=%d n_elig=%d (all >= 1)", d->M, d->T,
                d->n_utts, d->n_elig);
  if (d->C < 1 || d->max_tries < 1) return fail(CTN_ERR_ARG, "bad dynamic-mix descriptor C=%d max_tries=%d", d->C, d->max_tries);
  if ((d->pool_dtype != 0 && d->pool_dtype != 1) || (d->level_mode != 0 && d->level_mode != 1))
    return fail(CTN_ERR_ARG, "pool_dtype=%d level_mode=%d: each 0 or 1", d->pool_dtype, d->level_mode);
  if (!isfinite(d->level_lo_db) || !isfinite(d->level_hi_db) || !isfinite(d->peak) || d->peak < 0.f)
    return fail(CTN_ERR_ARG, "levels and peak must be finite, peak >= 0");
  if (d->C > DMIX_MAX_C) return fail(CTN_ERR_UNSUPPORTED, "C=%d > %d slots per row", d->C, DMIX_MAX_C);
  if (d->max_tries > DMIX_MAX_TRIES)
    return fail(CTN_ERR_UNSUPPORTED, "max_tries=%d > %d", d->max_tries, DMIX_MAX_TRIES);
  if (d->T > (1 << 30)) return fail(CTN_ERR_UNSUPPORTED, "T=%d > 2^30 samples", d->T);
  const long nchunk = ((long)d->T + DMIX_CHUNK - 1) / DMIX_CHUNK;
  if ((long)d->M * d->C > INT32_MAX / nchunk)
    return fail(CTN_ERR_UNSUPPORTED, "M*C*ceil(T/%d) = %ld*%ld workgroups exceed one grid", DMIX_CHUNK,
                (long)d->M * d->C, nchunk);
  return CTN_OK;
}

extern "C" size_t ctn_dmix_workspace_bytes(const ctn_dmix_desc* d) {
  if (dmix_check(d) != CTN_OK) return 0;
  return dmix_layout(d->M, d->C, d->T).bytes;
}

static DmixDrawArgs dmix_draw_args(const ctn_dmix_desc* d, const int64_t* off, const int32_t* spk, const int32_t* elig,
                                   int64_t first_sample, int64_t* first_sample_dev, int64_t advance,
                                   ctn_dmix_entry* plan) {
  DmixDrawArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.U = d->n_utts; a.E = d->n_elig; a.max_tries = d->max_tries;
  a.lo_db = d->level_lo_db; a.hi_db = d->level_hi_db;
  a.seed_lo = (uint32_t)d->seed; a.seed_hi = (uint32_t)(d->seed >> 32);
  a.off = off; a.spk = spk; a.elig = elig;
  a.first = first_sample; a.first_dev = first_sample_dev; a.advance = advance;
  a.plan = reinterpret_cast<DmixEntry*>(plan);
  return a;
}

extern "C" int ctn_dmix_draw(const ctn_dmix_desc* d, const int64_t* off, const int32_t* spk, const int32_t* elig,
                             int64_t first_sample, int64_t* first_sample_dev, int64_t advance, ctn_dmix_entry* plan,
                             void* stream) {
  if (int rc = dmix_check(d)) return rc;
  if (!off || !spk || !elig || !plan) return fail(CTN_ERR_ARG, "null pointer");
  const DmixDrawArgs a = dmix_draw_args(d, off, spk, elig, first_sample, first_sample_dev, advance, plan);
  CTN_HIP(launch_dmix_draw(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_dmix_mix(const ctn_dmix_desc* d, const void* pool, const int64_t* off, const ctn_dmix_entry* plan,
                            float* gains, float* sources, float* mixture, int32_t* status, void* ws, size_t ws_bytes,
                            void* stream) {
  if (int rc = dmix_check(d)) return rc;
  if (!pool || !off || !plan || !gains || !sources || !mixture || !status) return fail(CTN_ERR_ARG, "null pointer");
  if ((uintptr_t)pool % (d->pool_dtype == 0 ? 2 : 4) || (uintptr_t)sources % 4 || (uintptr_t)mixture % 4)
    return fail(CTN_ERR_ARG, "pool, sources or mixture is not aligned to its element size");
  DmixMixArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.U = d->n_utts; a.pool_dtype = d->pool_dtype; a.level_mode = d->level_mode;
  a.peak = d->peak;
  a.L = dmix_layout(d->M, d->C, d->T);
  if (!ws || ws_bytes < a.L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, a.L.bytes);
  if ((uintptr_t)ws % 8) return fail(CTN_ERR_ARG, "workspace is not 8-byte aligned");
  a.pool = pool; a.off = off; a.plan = reinterpret_cast<const DmixEntry*>(plan);
  a.gains = gains; a.sources = sources; a.mixture = mixture; a.status = status;
  a.ws = reinterpret_cast<char*>(ws);
  CTN_HIP(launch_dmix_mix(a, (hipStream_t)stream));
  return CTN_OK;
}

// Speed perturbation: ctn_dmix_draw_sp, ctn_dmix_mix_sp
static_assert(sizeof(ctn_dmix_speeds) == 68, "ctn_dmix_speeds layout");

// Validates the table against the descriptor's T and fills the kernels' form of it.
static int dmix_speeds_check(const ctn_dmix_speeds* sp, int T, DmixSpeedTable* out) {
  if (!sp) return fail(CTN_ERR_ARG, "null speed table");
  if (sp->n < 1) return fail(CTN_ERR_ARG, "speed table with n=%d entries (1..%d)", sp->n, DMIX_MAX_SPEEDS);
  if (sp->n > DMIX_MAX_SPEEDS)
    return fail(CTN_ERR_UNSUPPORTED, "speed table with n=%d > %d entries", sp->n, DMIX_MAX_SPEEDS);
  int32_t foff = 0;
  out->n = sp->n;
  for (int k = 0; k < sp->n; ++k) {
    const int up = sp->r[k].up, down = sp->r[k].down;
    if (up < 1 || down < 1) return fail(CTN_ERR_ARG, "speed %d: ratio %d/%d (both >= 1)", k, up, down);
    if (up > DMIX_MAX_RATIO || down > DMIX_MAX_RATIO)
      return fail(CTN_ERR_UNSUPPORTED, "speed %d: ratio %d/%d beyond %d", k, up, down, DMIX_MAX_RATIO);
    int a = up, b = down;
    while (b) { const int t = a % b; a = b; b = t; }
    if (a != 1) return fail(CTN_ERR_ARG, "speed %d: ratio %d/%d is not reduced", k, up, down);
    if (up > 2 * down || down > 2 * up)
      return fail(CTN_ERR_UNSUPPORTED, "speed %d: ratio %d/%d outside [1/2, 2]", k, up, down);
    DmixSpeed& s = out->s[k];
    s.up = up; s.down = down; s.hl = 10 * (up > down ? up : down);
    s.foff = foff;
    s.span = (int64_t)(T - 1) * down / up + 1;
    if (up != 1 || down != 1) foff += 2 * s.hl + 1;
  }
  return CTN_OK;
}

extern "C" size_t ctn_dmix_sp_filter_floats(const ctn_dmix_speeds* sp) {
  DmixSpeedTable t{};
  if (dmix_speeds_check(sp, 1, &t) != CTN_OK) return 0;
  size_t n = 0;
  for (int k = 0; k < t.n; ++k)
    if (t.s[k].up != 1 || t.s[k].down != 1) n += 2 * (size_t)t.s[k].hl + 1;
  return n;
}

extern "C" size_t ctn_dmix_sp_workspace_bytes(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp) {
  DmixSpeedTable t{};
  if (dmix_check(d) != CTN_OK || dmix_speeds_check(sp, d->T, &t) != CTN_OK) return 0;
  return dmix_sp_layout(d->M, d->C, d->T).bytes;
}

extern "C" int ctn_dmix_draw_sp(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp, const int64_t* off,
                                const int32_t* spk, const int32_t* elig, int64_t first_sample,
                                int64_t* first_sample_dev, int64_t advance, ctn_dmix_entry* plan, int32_t* speed,
                                void* stream) {
  if (int rc = dmix_check(d)) return rc;
  DmixSpeedTable t{};
  if (int rc = dmix_speeds_check(sp, d->T, &t)) return rc;
  if (!off || !spk || !elig || !plan || !speed) return fail(CTN_ERR_ARG, "null pointer");
  DmixDrawArgs a = dmix_draw_args(d, off, spk, elig, first_sample, first_sample_dev, advance, plan);
  a.speed = speed; a.nspeed = t.n;
  for (int k = 0; k < t.n; ++k) a.span[k] = t.s[k].span;
  CTN_HIP(launch_dmix_draw(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_dmix_mix_sp(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp, const float* filt, const void* pool,
                               const int64_t* off, const ctn_dmix_entry* plan, const int32_t* speed, float* gains,
                               float* sources, float* mixture, int32_t* status, void* ws, size_t ws_bytes,
                               void* stream) {
  if (int rc = dmix_check(d)) return rc;
  DmixResampleArgs r{};
  if (int rc = dmix_speeds_check(sp, d->T, &r.sp)) return rc;
  if (!pool || !off || !plan || !speed || !gains || !sources || !mixture || !status)
    return fail(CTN_ERR_ARG, "null pointer");
  if (!filt && ctn_dmix_sp_filter_floats(sp) > 0) return fail(CTN_ERR_ARG, "null pointer (filter table)");
  if ((uintptr_t)pool % (d->pool_dtype == 0 ? 2 : 4) || (uintptr_t)sources % 4 || (uintptr_t)mixture % 4 ||
      (uintptr_t)filt % 4)
    return fail(CTN_ERR_ARG, "pool, filter table, sources or mixture is not aligned to its element size");
  r.L = dmix_sp_layout(d->M, d->C, d->T);
  if (!ws || ws_bytes < r.L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, r.L.bytes);
  if ((uintptr_t)ws % 16) return fail(CTN_ERR_ARG, "workspace is not 16-byte aligned");
  r.M = d->M; r.C = d->C; r.T = d->T; r.U = d->n_utts; r.pool_dtype = d->pool_dtype;
  r.filt = filt; r.pool = pool; r.off = off; r.plan = reinterpret_cast<const DmixEntry*>(plan); r.speed = speed;
  r.ws = reinterpret_cast<char*>(ws);
  DmixMixArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.level_mode = d->level_mode; a.peak = d->peak;
  a.gains = gains; a.sources = sources; a.mixture = mixture; a.status = status;
  CTN_HIP(launch_dmix_mix_sp(r, a, (hipStream_t)stream));
  return CTN_OK;
}
