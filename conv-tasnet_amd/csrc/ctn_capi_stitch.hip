// C-ABI entries of windowed separation (include/ctn.h ctn_stitch_*).
#include "ctn_capi_util.h"
#include "ctn_stitch.h"

using namespace ctn;

static_assert(sizeof(ctn_stitch_desc) == 20, "ctn_stitch_desc layout");

// Every constraint is checked here, before the device is touched.
static int stitch_check(const ctn_stitch_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->C < STITCH_MIN_C || d->C > STITCH_MAX_C)
    return fail(CTN_ERR_ARG, "C=%d speakers (%d ... %d: the search is over all C! permutations)", d->C, STITCH_MIN_C,
                STITCH_MAX_C);
  if (d->W < 2 || d->O < 1 || d->O > d->W / 2)
    return fail(CTN_ERR_ARG, "window W=%d, overlap O=%d: 1 <= O <= W/2", d->W, d->O);
  if (d->T < 1) return fail(CTN_ERR_ARG, "T=%d samples (>= 1)", d->T);
  if (d->T > (1 << 30) || d->W > (1 << 30)) return fail(CTN_ERR_ARG, "T=%d, W=%d beyond 2^30 samples", d->T, d->W);
  const int J = stitch_window_count(d->T, d->W, d->W - d->O);
  if (d->J != J) return fail(CTN_ERR_ARG, "J=%d windows; T=%d W=%d O=%d give %d", d->J, d->T, d->W, d->O, J);
  return CTN_OK;
}

static size_t stitch_ws_bytes(const ctn_stitch_desc* d) {
  const size_t nb = d->J > 1 ? (size_t)(d->J - 1) : 1;
  return nb * (size_t)stitch_nchunk(d->O) * d->C * d->C * sizeof(double);
}

static StitchArgs stitch_args(const ctn_stitch_desc* d) {
  StitchArgs a{};
  a.J = d->J; a.C = d->C; a.W = d->W; a.O = d->O; a.T = d->T; a.Hs = d->W - d->O;
  a.nchunk = stitch_nchunk(d->O);
  a.vec = d->W % 4 == 0 && d->O % 4 == 0;
  return a;
}

extern "C" size_t ctn_stitch_workspace_bytes(const ctn_stitch_desc* d) {
  if (stitch_check(d) != CTN_OK) return 0;
  return stitch_ws_bytes(d);
}

extern "C" int ctn_stitch_frame(const ctn_stitch_desc* d, const float* x, float* win, void* stream) {
  if (int rc = stitch_check(d)) return rc;
  if (!x || !win) return fail(CTN_ERR_ARG, "null pointer");
  if ((uintptr_t)x % 4 || (uintptr_t)win % 4) return fail(CTN_ERR_ARG, "x or win is not aligned to its element size");
  StitchArgs a = stitch_args(d);
  a.vec = a.vec && (uintptr_t)x % 16 == 0 && (uintptr_t)win % 16 == 0;
  a.x = x; a.win = win;
  CTN_HIP(launch_stitch_frame(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_stitch_plan(const ctn_stitch_desc* d, const float* P, double* sim, int32_t* perm, int32_t* sigma,
                               int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = stitch_check(d)) return rc;
  if (!P || !sim || !perm || !sigma || !status) return fail(CTN_ERR_ARG, "null pointer");
  if ((uintptr_t)P % 4 || (uintptr_t)sim % 8 || (uintptr_t)perm % 4 || (uintptr_t)sigma % 4 || (uintptr_t)status % 4)
    return fail(CTN_ERR_ARG, "P, sim, perm, sigma or status is not aligned to its element size");
  const size_t need = stitch_ws_bytes(d);
  if (!ws || ws_bytes < need) return fail(CTN_ERR_ARG, "workspace %zu < %zu", ws_bytes, need);
  if ((uintptr_t)ws % 8) return fail(CTN_ERR_ARG, "workspace is not 8-byte aligned");
  StitchArgs a = stitch_args(d);
  a.vec = a.vec && (uintptr_t)P % 16 == 0;
  a.P = P; a.part = reinterpret_cast<double*>(ws);
  a.sim = sim; a.perm = perm; a.sigma = sigma; a.status = status;
  CTN_HIP(launch_stitch_plan(a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_stitch_ola(const ctn_stitch_desc* d, const float* P, const int32_t* sigma, const float* fade,
                              float* out, void* stream) {
  if (int rc = stitch_check(d)) return rc;
  if (!P || !sigma || !fade || !out) return fail(CTN_ERR_ARG, "null pointer");
  if ((uintptr_t)P % 4 || (uintptr_t)sigma % 4 || (uintptr_t)fade % 4 || (uintptr_t)out % 4)
    return fail(CTN_ERR_ARG, "P, sigma, fade or out is not aligned to its element size");
  StitchArgs a = stitch_args(d);
  a.vec = a.vec && (uintptr_t)P % 16 == 0 && (uintptr_t)fade % 16 == 0;
  a.vec_out = a.vec && d->T % 4 == 0 && (uintptr_t)out % 16 == 0;
  a.P = P; a.sigma_in = sigma; a.fade = fade; a.out = out;
  CTN_HIP(launch_stitch_ola(a, (hipStream_t)stream));
  return CTN_OK;
}
