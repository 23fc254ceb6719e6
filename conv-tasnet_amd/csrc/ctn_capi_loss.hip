// C-ABI entries of PIT SI-SNR loss, MixIT loss and BSS Eval energies (include/ctn.h ctn_pit_*,
// ctn_mixit_*, ctn_bss_*).
#include "ctn_capi_util.h"
#include "ctn_bss.h"
#include "ctn_codec.h"
#include "ctn_mixit.h"

using namespace ctn;

// ===========================================================================
// PIT SI-SNR loss
// ===========================================================================
static int pit_chunks(int T) {
  int c = (T + 2047) / 2048;
  return c < 1 ? 1 : (c > 64 ? 64 : c);
}

constexpr int PIT_CMAX = 16;   // C <= 10: all C! permutations; 11..16: assignment (ctn_pit.hip)

static void pit_perms(PitArgs& a) {
  int p[4] = {0, 1, 2, 3};
  a.nperm = 0;
  if (a.C > 4) return;          // pit_final_wide decodes them on the device
  // lexicographic order == itertools.permutations(range(C)) (pit_criterion.py:66)
  do {
    for (int i = 0; i < a.C; ++i) a.perms[a.nperm][i] = p[i];
    ++a.nperm;
    int i = a.C - 2;
    while (i >= 0 && p[i] >= p[i + 1]) --i;
    if (i < 0) break;
    int j = a.C - 1;
    while (p[j] <= p[i]) --j;
    int t = p[i]; p[i] = p[j]; p[j] = t;
    for (int l = i + 1, r = a.C - 1; l < r; ++l, --r) { t = p[l]; p[l] = p[r]; p[r] = t; }
  } while (true);
}

extern "C" size_t ctn_pit_workspace_bytes(const ctn_pit_desc* d) {
  if (!d || d->M < 1 || d->C < 1 || d->C > PIT_CMAX || d->T < 1) return 0;
  return (size_t)d->M * pit_chunks(d->T) * pit_nv(d->C) * sizeof(double) + (size_t)d->M * sizeof(double) + 256;
}

extern "C" int ctn_pit_forward(const ctn_pit_desc* d, const float* source, float* est, const int64_t* lengths,
                               float* loss, float* max_snr, int64_t* best_perm, float* reordered, float* coef,
                               void* ws, size_t ws_bytes, void* stream) {
  if (!d || d->M < 1 || d->C < 1 || d->T < 1) return fail(CTN_ERR_ARG, "bad PIT descriptor");
  if (d->C > PIT_CMAX) return fail(CTN_ERR_UNSUPPORTED, "C=%d > %d speakers", d->C, PIT_CMAX);
  if (!source || !est || !lengths || !loss || !max_snr || !best_perm || !coef) return fail(CTN_ERR_ARG, "null pointer");
  if (!ws || ws_bytes < ctn_pit_workspace_bytes(d)) return fail(CTN_ERR_WORKSPACE, "PIT workspace too small");
  PitArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T;
  a.src = source; a.est = est; a.lengths = lengths;
  a.slab = reinterpret_cast<double*>(ws);
  a.chunks = pit_chunks(d->T);
  a.msd = a.slab + (size_t)d->M * a.chunks * pit_nv(d->C);
  a.max_snr = max_snr; a.best = best_perm; a.coef = coef; a.loss = loss;
  a.est_inplace = est; a.reordered = reordered;
  pit_perms(a);
  CTN_HIP(launch_pit_forward(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_pit_backward(const ctn_pit_desc* d, const float* source, const float* est,
                                const int64_t* lengths, const float* coef, const float* g_loss,
                                const float* g_max_snr, float* g_est, void* stream) {
  if (!d || d->M < 1 || d->C < 1 || d->T < 1) return fail(CTN_ERR_ARG, "bad PIT descriptor");
  if (d->C > PIT_CMAX) return fail(CTN_ERR_UNSUPPORTED, "C=%d > %d speakers", d->C, PIT_CMAX);
  if (!source || !est || !lengths || !coef || !g_est) return fail(CTN_ERR_ARG, "null pointer");
  PitArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T;
  a.src = source; a.est = est; a.lengths = lengths; a.coef = const_cast<float*>(coef);
  a.g_loss = g_loss; a.g_maxsnr = g_max_snr; a.gest = g_est;
  CTN_HIP(launch_pit_backward(a, (hipStream_t)stream));
  return CTN_OK;
}

// ===========================================================================
// MixIT loss, ctn_mixit.hip (the chunk rule of the PIT statistics)
// ===========================================================================
static int mixit_check(const ctn_mixit_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->T < 1) return fail(CTN_ERR_ARG, "bad MixIT descriptor M=%d T=%d (both >= 1)", d->M, d->T);
  if (d->C < MIXIT_CMIN || d->C > MIXIT_CMAX)
    return fail(CTN_ERR_UNSUPPORTED, "MixIT with C=%d outputs (%d to %d)", d->C, MIXIT_CMIN, MIXIT_CMAX);
  if (d->mode != CTN_MIXIT_SNR && d->mode != CTN_MIXIT_SI_SNR)
    return fail(CTN_ERR_ARG, "unknown MixIT mode %d (0 snr, 1 si_snr)", d->mode);
  if (!isfinite(d->snr_max)) return fail(CTN_ERR_ARG, "MixIT snr_max is not finite");
  return CTN_OK;
}

static MixitArgs mixit_args(const ctn_mixit_desc* d) {
  MixitArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.mode = d->mode;
  a.tau = pow(10.0, -(double)d->snr_max / 10.0);
  a.chunks = pit_chunks(d->T);
  return a;
}

extern "C" size_t ctn_mixit_workspace_bytes(const ctn_mixit_desc* d) {
  if (mixit_check(d) != CTN_OK) return 0;
  return (size_t)d->M * pit_chunks(d->T) * mixit_nv(d->C) * sizeof(double) + (size_t)d->M * sizeof(double) + 256;
}

extern "C" int ctn_mixit_forward(const ctn_mixit_desc* d, const float* mixtures, const float* est,
                                 const int64_t* lengths, float* loss, float* max_snr, int64_t* assign, float* remix,
                                 float* coef, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = mixit_check(d)) return rc;
  if (!mixtures || !est || !lengths || !loss || !max_snr || !assign || !coef) return fail(CTN_ERR_ARG, "null pointer");
  if (!ws || ws_bytes < ctn_mixit_workspace_bytes(d)) return fail(CTN_ERR_WORKSPACE, "MixIT workspace too small");
  MixitArgs a = mixit_args(d);
  a.mix = mixtures; a.est = est; a.lengths = lengths;
  a.slab = reinterpret_cast<double*>(ws);
  a.msd = a.slab + (size_t)d->M * a.chunks * mixit_nv(d->C);
  a.loss = loss; a.max_snr = max_snr; a.assign = assign; a.coef = coef; a.remix = remix;
  CTN_HIP(launch_mixit_forward(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_mixit_backward(const ctn_mixit_desc* d, const float* mixtures, const float* est,
                                  const int64_t* lengths, const int64_t* assign, const float* coef,
                                  const float* g_loss, const float* g_max_snr, float* g_est, void* stream) {
  if (int rc = mixit_check(d)) return rc;
  if (!mixtures || !est || !lengths || !assign || !coef || !g_est) return fail(CTN_ERR_ARG, "null pointer");
  MixitArgs a = mixit_args(d);
  a.mix = mixtures; a.est = est; a.lengths = lengths;
  a.assign = const_cast<int64_t*>(assign); a.coef = const_cast<float*>(coef);
  a.g_loss = g_loss; a.g_maxsnr = g_max_snr; a.gest = g_est;
  CTN_HIP(launch_mixit_backward(a, (hipStream_t)stream));
  return CTN_OK;
}

// ===========================================================================
// BSS Eval v3 energies, ctn_bss.hip
// ===========================================================================
static int bss_check(const ctn_bss_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->C < 1 || d->E < 1 || d->flen < 1)
    return fail(CTN_ERR_ARG, "bad BSS descriptor M=%d C=%d E=%d flen=%d (all >= 1)", d->M, d->C, d->E, d->flen);
  if (d->T < d->flen) return fail(CTN_ERR_ARG, "T=%d samples are shorter than the %d-tap filters", d->T, d->flen);
  if ((long)d->C * d->flen > BSS_MAX_ORDER)
    return fail(CTN_ERR_UNSUPPORTED, "C*flen = %ld > %d (largest normal-equation system)", (long)d->C * d->flen,
                BSS_MAX_ORDER);
  if (d->M > BSS_MAX_M || d->E > BSS_MAX_M)
    return fail(CTN_ERR_UNSUPPORTED, "M=%d E=%d: at most %d each per call", d->M, d->E, BSS_MAX_M);
  return CTN_OK;
}

extern "C" size_t ctn_bss_workspace_bytes(const ctn_bss_desc* d) {
  if (bss_check(d) != CTN_OK) return 0;
  return bss_layout(d->M, d->C, d->E, d->T, d->flen).bytes;
}

extern "C" int ctn_bss_eval(const ctn_bss_desc* d, const float* refs, const float* sigs, const int32_t* lengths,
                            double* energies, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = bss_check(d)) return rc;
  if (!refs || !sigs || !lengths || !energies || !status) return fail(CTN_ERR_ARG, "null pointer");
  BssArgs a{};
  a.M = d->M; a.C = d->C; a.E = d->E; a.T = d->T; a.flen = d->flen;
  a.L = bss_layout(d->M, d->C, d->E, d->T, d->flen);
  if (!ws || ws_bytes < a.L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, a.L.bytes);
  a.refs = refs; a.sigs = sigs; a.lengths = lengths; a.energies = energies; a.status = status;
  a.ws = reinterpret_cast<double*>(ws);
  CTN_HIP(launch_bss_eval(a, (hipStream_t)stream));
  return CTN_OK;
}
