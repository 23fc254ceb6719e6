// C-ABI entries of the PIT loss with silent sources (include/ctn.h ctn_pitvar_*).
#include "ctn_capi_util.h"
#include "ctn_pitvar.h"

using namespace ctn;

// the chunk rule of the PIT and MixIT statistics
static int pitvar_chunks(int T) {
  int c = (T + 2047) / 2048;
  return c < 1 ? 1 : (c > 64 ? 64 : c);
}

static int pitvar_check(const ctn_pitvar_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->T < 1) return fail(CTN_ERR_ARG, "bad PIT-var descriptor M=%d T=%d (both >= 1)", d->M, d->T);
  if (d->C < PITVAR_CMIN || d->C > PITVAR_CMAX)
    return fail(CTN_ERR_UNSUPPORTED, "PIT with silent sources for C=%d outputs (%d to %d)", d->C, PITVAR_CMIN,
                PITVAR_CMAX);
  if (d->mode != CTN_PITVAR_SNR && d->mode != CTN_PITVAR_SI_SNR)
    return fail(CTN_ERR_ARG, "unknown PIT-var mode %d (0 snr, 1 si_snr)", d->mode);
  if (!isfinite(d->snr_max) || !isfinite(d->inactive_snr_max))
    return fail(CTN_ERR_ARG, "PIT-var snr_max or inactive_snr_max is not finite");
  return CTN_OK;
}

static PitVarArgs pitvar_args(const ctn_pitvar_desc* d) {
  PitVarArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.mode = d->mode;
  a.tau = pow(10.0, -(double)d->snr_max / 10.0);
  a.tau0 = pow(10.0, -(double)d->inactive_snr_max / 10.0);
  a.chunks = pitvar_chunks(d->T);
  return a;
}

extern "C" size_t ctn_pitvar_workspace_bytes(const ctn_pitvar_desc* d) {
  if (pitvar_check(d) != CTN_OK) return 0;
  return (size_t)d->M * pitvar_chunks(d->T) * pitvar_nv(d->C) * sizeof(double) + (size_t)d->M * sizeof(double) + 256;
}

extern "C" int ctn_pitvar_forward(const ctn_pitvar_desc* d, const float* source, const float* est,
                                  const float* mixture, const int64_t* lengths, float* loss, float* max_snr,
                                  int64_t* perm, uint8_t* active, float* coef, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (int rc = pitvar_check(d)) return rc;
  if (!source || !est || !lengths || !loss || !max_snr || !perm || !active || !coef)
    return fail(CTN_ERR_ARG, "null pointer");
  if (!ws || ws_bytes < ctn_pitvar_workspace_bytes(d)) return fail(CTN_ERR_WORKSPACE, "PIT-var workspace too small");
  PitVarArgs a = pitvar_args(d);
  a.src = source; a.est = est; a.mix = mixture; a.lengths = lengths;
  a.slab = reinterpret_cast<double*>(ws);
  a.msd = a.slab + (size_t)d->M * a.chunks * pitvar_nv(d->C);
  a.loss = loss; a.max_snr = max_snr; a.perm = perm; a.active = active; a.coef = coef;
  CTN_HIP(launch_pitvar_forward(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_pitvar_backward(const ctn_pitvar_desc* d, const float* source, const float* est,
                                   const int64_t* lengths, const float* coef, const float* g_loss,
                                   const float* g_max_snr, float* g_est, void* stream) {
  if (int rc = pitvar_check(d)) return rc;
  if (!source || !est || !lengths || !coef || !g_est) return fail(CTN_ERR_ARG, "null pointer");
  PitVarArgs a = pitvar_args(d);
  a.src = source; a.est = est; a.lengths = lengths; a.coef = const_cast<float*>(coef);
  a.g_loss = g_loss; a.g_maxsnr = g_max_snr; a.gest = g_est;
  CTN_HIP(launch_pitvar_backward(a, (hipStream_t)stream));
  return CTN_OK;
}
