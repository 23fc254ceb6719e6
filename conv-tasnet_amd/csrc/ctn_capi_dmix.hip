// C-ABI entries of dynamic mixing (include/ctn.h ctn_dmix_*).
#include "ctn_capi_util.h"
#include "ctn_dmix.h"
#include "ctn_dmix_aug.h"

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

extern "C" int ctn_dmix_thin(const ctn_dmix_desc* d, int32_t min_speakers, int64_t first_sample,
                             const int64_t* first_sample_dev, int64_t drawn_advance, ctn_dmix_entry* plan,
                             int32_t* count, void* stream) {
  if (int rc = dmix_check(d)) return rc;
  if (min_speakers < 1 || min_speakers > d->C)
    return fail(CTN_ERR_ARG, "min_speakers=%d outside 1..C=%d", min_speakers, d->C);
  if (!plan || !count) return fail(CTN_ERR_ARG, "null pointer");
  DmixThinArgs a{};
  a.M = d->M; a.C = d->C; a.min_speakers = min_speakers;
  a.seed_lo = (uint32_t)d->seed; a.seed_hi = (uint32_t)(d->seed >> 32);
  a.first = first_sample; a.first_dev = first_sample_dev; a.back = drawn_advance;
  a.plan = reinterpret_cast<DmixEntry*>(plan); a.count = count;
  CTN_HIP(launch_dmix_thin(a, (hipStream_t)stream));
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

// Reverberation and noise: ctn_dmix_draw_aug, ctn_dmix_mix_aug (ctn_dmix_aug.hip)
static_assert(sizeof(ctn_dmix_aug) == 32, "ctn_dmix_aug layout");

static int dmix_aug_check(const ctn_dmix_desc* d, const ctn_dmix_aug* g) {
  if (!g) return fail(CTN_ERR_ARG, "null augmentation descriptor");
  if (g->n_rirs < 0 || g->n_noise_utts < 0 || g->n_noise_elig < 0 || (g->n_noise_utts > 0) != (g->n_noise_elig > 0))
    return fail(CTN_ERR_ARG, "bad augmentation descriptor n_rirs=%d n_noise_utts=%d n_noise_elig=%d", g->n_rirs,
                g->n_noise_utts, g->n_noise_elig);
  if (g->n_rirs > 0) {
    if (!(g->rir_prob >= 0.f && g->rir_prob <= 1.f)) return fail(CTN_ERR_ARG, "rir_prob=%g outside [0, 1]", g->rir_prob);
    if (g->rir_max_taps < 1) return fail(CTN_ERR_ARG, "rir_max_taps=%d (>= 1)", g->rir_max_taps);
    if (g->rir_max_taps > DMIX_MAX_RIR_TAPS)
      return fail(CTN_ERR_UNSUPPORTED, "rir_max_taps=%d > %d taps (limits)", g->rir_max_taps, DMIX_MAX_RIR_TAPS);
  }
  if (g->n_noise_utts > 0) {
    if (g->noise_dtype != 0 && g->noise_dtype != 1) return fail(CTN_ERR_ARG, "noise_dtype=%d: 0 or 1", g->noise_dtype);
    if (!isfinite(g->snr_lo_db) || !isfinite(g->snr_hi_db)) return fail(CTN_ERR_ARG, "snr_lo_db and snr_hi_db must be finite");
    if (d->C + 1 > DMIX_MAX_C)
      return fail(CTN_ERR_UNSUPPORTED, "C=%d with noise: C + 1 > %d slots per row (limits)", d->C, DMIX_MAX_C);
  }
  return CTN_OK;
}

// d, the optional speed table and the augmentation descriptor; fills the table's kernel form.
static int dmix_aug_check_all(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp, const ctn_dmix_aug* g,
                              DmixSpeedTable* t) {
  if (int rc = dmix_check(d)) return rc;
  if (sp)
    if (int rc = dmix_speeds_check(sp, d->T, t)) return rc;
  return dmix_aug_check(d, g);
}

extern "C" size_t ctn_dmix_aug_workspace_bytes(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp, const ctn_dmix_aug* g) {
  DmixSpeedTable t{};
  if (dmix_aug_check_all(d, sp, g, &t) != CTN_OK) return 0;
  return dmix_aug_layout(d->M, d->C, d->T, sp != nullptr, g->n_rirs > 0, g->n_noise_utts > 0).bytes;
}

extern "C" int ctn_dmix_draw_aug(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp, const ctn_dmix_aug* g,
                                 const int64_t* off, const int32_t* spk, const int32_t* elig, const int64_t* noff,
                                 const int32_t* nelig, int64_t first_sample, int64_t* first_sample_dev,
                                 int64_t advance, ctn_dmix_entry* plan, int32_t* speed, int32_t* rir,
                                 ctn_dmix_entry* nplan, void* stream) {
  DmixSpeedTable t{};
  if (int rc = dmix_aug_check_all(d, sp, g, &t)) return rc;
  const bool noise = g->n_noise_utts > 0;
  if (!off || !spk || !elig || !plan || (g->n_rirs > 0 && !rir) || (sp && !speed) || (noise && (!noff || !nelig || !nplan)))
    return fail(CTN_ERR_ARG, "null pointer");
  DmixAugDrawArgs x{};
  x.M = d->M; x.C = d->C; x.T = d->T;
  x.seed_lo = (uint32_t)d->seed; x.seed_hi = (uint32_t)(d->seed >> 32);
  x.first = first_sample; x.first_dev = first_sample_dev;
  x.n_rirs = g->n_rirs; x.rir_prob = g->rir_prob; x.rir = rir;
  if (noise) {
    x.NU = g->n_noise_utts; x.NE = g->n_noise_elig; x.noff = noff; x.nelig = nelig;
    x.snr_lo = g->snr_lo_db; x.snr_hi = g->snr_hi_db;
    x.nplan = reinterpret_cast<DmixEntry*>(nplan);
  }
  CTN_HIP(launch_dmix_draw_aug(x, (hipStream_t)stream));   // reads the device counter before it advances
  DmixDrawArgs a = dmix_draw_args(d, off, spk, elig, first_sample, first_sample_dev, advance, plan);
  if (sp) {
    a.speed = speed; a.nspeed = t.n;
    for (int k = 0; k < t.n; ++k) a.span[k] = t.s[k].span;
  }
  CTN_HIP(launch_dmix_draw(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_dmix_mix_aug(const ctn_dmix_desc* d, const ctn_dmix_speeds* sp, const ctn_dmix_aug* g,
                                const float* filt, const void* pool, const int64_t* off, const ctn_dmix_entry* plan,
                                const int32_t* speed, const float* rir_pool, const int64_t* roff, const int32_t* rir,
                                const void* noise_pool, const int64_t* noff, const ctn_dmix_entry* nplan, float* gains,
                                float* ngain, float* sources, float* mixture, float* noise_out, int32_t* status,
                                void* ws, size_t ws_bytes, void* stream) {
  DmixResampleArgs r{};
  if (int rc = dmix_aug_check_all(d, sp, g, &r.sp)) return rc;
  const bool rirs = g->n_rirs > 0, noise = g->n_noise_utts > 0;
  if (!pool || !off || !plan || !gains || !sources || !mixture || !status || (sp && !speed) ||
      (rirs && (!rir_pool || !roff || !rir)) || (noise && (!noise_pool || !noff || !nplan || !ngain)))
    return fail(CTN_ERR_ARG, "null pointer");
  if (sp && !filt && ctn_dmix_sp_filter_floats(sp) > 0) return fail(CTN_ERR_ARG, "null pointer (filter table)");
  if ((uintptr_t)pool % (d->pool_dtype == 0 ? 2 : 4) || (uintptr_t)sources % 4 || (uintptr_t)mixture % 4 ||
      (uintptr_t)filt % 4 || (uintptr_t)rir_pool % 4 || (uintptr_t)noise_out % 4 ||
      (noise && (uintptr_t)noise_pool % (g->noise_dtype == 0 ? 2 : 4)))
    return fail(CTN_ERR_ARG, "a pool, the filter table, sources, mixture or noise_out is not aligned to its element size");
  if ((uintptr_t)roff % 8 || (uintptr_t)noff % 8 || (uintptr_t)off % 8)
    return fail(CTN_ERR_ARG, "an offset table is not aligned to 8 bytes");
  const DmixAugLayout L = dmix_aug_layout(d->M, d->C, d->T, sp != nullptr, rirs, noise);
  if (!ws || ws_bytes < L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, L.bytes);
  if ((uintptr_t)ws % 16) return fail(CTN_ERR_ARG, "workspace is not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  DmixMixArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.U = d->n_utts; a.pool_dtype = d->pool_dtype; a.level_mode = d->level_mode;
  a.peak = d->peak;
  a.pool = pool; a.off = off; a.plan = reinterpret_cast<const DmixEntry*>(plan);
  a.gains = gains; a.sources = sources; a.mixture = mixture; a.status = status;
  a.ws = reinterpret_cast<char*>(ws);
  a.L = L.sp.mix;
  if (sp) {
    r.L = L.sp;
    r.M = d->M; r.C = d->C; r.T = d->T; r.U = d->n_utts; r.pool_dtype = d->pool_dtype;
    r.filt = filt; r.pool = pool; r.off = off; r.plan = a.plan; r.speed = speed;
    r.ws = a.ws;
    CTN_HIP(launch_dmix_resample(r, &a, s));
  }
  if (rirs) {
    DmixReverbArgs v{};
    v.M = d->M; v.C = d->C; v.T = d->T; v.U = a.U; v.pool_dtype = a.pool_dtype;
    v.pool = a.pool; v.off = a.off; v.plan = a.plan;
    v.n_rirs = g->n_rirs; v.max_taps = g->rir_max_taps;
    v.rir_pool = rir_pool; v.roff = roff; v.rir = rir;
    v.ws = a.ws; v.L = L;
    CTN_HIP(launch_dmix_reverb(v, &a, s));
  }
  if (!noise) {
    CTN_HIP(launch_dmix_mix(a, s));
    return CTN_OK;
  }
  DmixNoiseArgs nz{};
  nz.NU = g->n_noise_utts; nz.dtype = g->noise_dtype;
  nz.pool = noise_pool; nz.off = noff; nz.nplan = reinterpret_cast<const DmixEntry*>(nplan);
  nz.ngain = ngain; nz.noise_out = noise_out;
  nz.off_pw = L.off_pw; nz.off_ng0 = L.off_ng0;
  CTN_HIP(launch_dmix_mix_noise(a, nz, s));
  return CTN_OK;
}
