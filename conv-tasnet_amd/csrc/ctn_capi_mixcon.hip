// C-ABI entries of the mixture-consistency projection (include/ctn.h ctn_mixcon_*).
#include "ctn_capi_util.h"
#include "ctn_mixcon.h"

using namespace ctn;

// the chunk rule of the PIT and MixIT statistics
static int mixcon_chunks(int T) {
  int c = (T + 2047) / 2048;
  return c < 1 ? 1 : (c > 64 ? 64 : c);
}

static int mixcon_check(const ctn_mixcon_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->T < 1)
    return fail(CTN_ERR_ARG, "bad mixture-consistency descriptor M=%d T=%d (both >= 1)", d->M, d->T);
  if (d->mode != CTN_MIXCON_UNIFORM && d->mode != CTN_MIXCON_POWER)
    return fail(CTN_ERR_ARG, "unknown mixture-consistency mode %d (0 uniform, 1 power)", d->mode);
  if (d->C < MIXCON_CMIN || d->C > MIXCON_CMAX)
    return fail(CTN_ERR_UNSUPPORTED, "mixture consistency with C=%d outputs (%d to %d)", d->C, MIXCON_CMIN,
                MIXCON_CMAX);
  if (d->M > (1 << 22) || d->T > (1 << 30))
    return fail(CTN_ERR_UNSUPPORTED, "mixture consistency with M=%d T=%d (at most 2^22 and 2^30)", d->M, d->T);
  return CTN_OK;
}

static MixconArgs mixcon_args(const ctn_mixcon_desc* d, void* ws) {
  MixconArgs a{};
  a.M = d->M; a.C = d->C; a.T = d->T; a.mode = d->mode;
  a.chunks = mixcon_chunks(d->T);
  a.slab = reinterpret_cast<double*>(ws);
  a.kcoef = a.slab + (size_t)d->M * a.chunks * d->C;
  return a;
}

extern "C" size_t ctn_mixcon_workspace_bytes(const ctn_mixcon_desc* d) {
  if (mixcon_check(d) != CTN_OK) return 0;
  return ((size_t)d->M * mixcon_chunks(d->T) * d->C + (size_t)d->M * d->C) * sizeof(double) + 256;
}

extern "C" int ctn_mixcon_forward(const ctn_mixcon_desc* d, const float* mixture, const float* est,
                                  const int64_t* lengths, float* out, double* coef, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (int rc = mixcon_check(d)) return rc;
  if (!mixture || !est || !out || (d->mode == CTN_MIXCON_POWER && !coef)) return fail(CTN_ERR_ARG, "null pointer");
  if (out == est) return fail(CTN_ERR_ARG, "mixture consistency is not done in place");
  if (!ws || ws_bytes < ctn_mixcon_workspace_bytes(d))
    return fail(CTN_ERR_WORKSPACE, "mixture-consistency workspace too small");
  MixconArgs a = mixcon_args(d, ws);
  a.x = mixture; a.s = est; a.lengths = lengths; a.y = out; a.coef = coef;
  CTN_HIP(launch_mixcon_forward(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_mixcon_backward(const ctn_mixcon_desc* d, const float* mixture, const float* est,
                                   const int64_t* lengths, const double* coef, const float* g_out, float* g_est,
                                   float* g_mixture, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = mixcon_check(d)) return rc;
  if (!g_out || !g_est || (d->mode == CTN_MIXCON_POWER && (!mixture || !est || !coef)))
    return fail(CTN_ERR_ARG, "null pointer");
  if (!ws || ws_bytes < ctn_mixcon_workspace_bytes(d))
    return fail(CTN_ERR_WORKSPACE, "mixture-consistency workspace too small");
  MixconArgs a = mixcon_args(d, ws);
  a.x = mixture; a.s = est; a.lengths = lengths; a.coef = const_cast<double*>(coef);
  a.g = g_out; a.gs = g_est; a.gx = g_mixture;
  CTN_HIP(launch_mixcon_backward(a, (hipStream_t)stream));
  return CTN_OK;
}
