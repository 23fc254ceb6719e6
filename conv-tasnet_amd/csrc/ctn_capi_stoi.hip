// C-ABI entries of STOI / ESTOI on the device (include/ctn.h ctn_stoi_*), ctn_stoi.hip.
#include "ctn_capi_util.h"
#include "ctn_stoi.h"

using namespace ctn;

static int stoi_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int stoi_check(const ctn_stoi_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->C < 1 || d->E < 1 || d->T < 1)
    return fail(CTN_ERR_ARG, "bad STOI descriptor M=%d C=%d E=%d T=%d (all >= 1)", d->M, d->C, d->E, d->T);
  if (d->up < 1 || d->down < 1 || stoi_gcd(d->up, d->down) != 1)
    return fail(CTN_ERR_ARG, "bad STOI ratio %d/%d (both >= 1 and reduced)", d->up, d->down);
  if (d->up != d->down && d->Hl < 1) return fail(CTN_ERR_ARG, "bad STOI filter half length Hl=%d (>= 1)", d->Hl);
  if (d->M > STOI_MAX_M || d->E > STOI_MAX_M)
    return fail(CTN_ERR_UNSUPPORTED, "M=%d E=%d: at most %d each per call", d->M, d->E, STOI_MAX_M);
  if (d->C > STOI_MAX_C) return fail(CTN_ERR_UNSUPPORTED, "C=%d > %d references", d->C, STOI_MAX_C);
  if (d->up > STOI_MAX_RATIO || d->down > STOI_MAX_RATIO)
    return fail(CTN_ERR_UNSUPPORTED, "ratio %d/%d: up and down at most %d", d->up, d->down, STOI_MAX_RATIO);
  if (d->up != d->down && d->Hl > STOI_MAX_HL)
    return fail(CTN_ERR_UNSUPPORTED, "filter half length Hl=%d > %d", d->Hl, STOI_MAX_HL);
  if (((long)d->T * d->up + d->down - 1) / d->down > 0x7fffffffL)
    return fail(CTN_ERR_UNSUPPORTED, "T=%d at %d/%d: more than 2^31 - 1 resampled samples", d->T, d->up, d->down);
  return CTN_OK;
}

extern "C" size_t ctn_stoi_table_doubles(const ctn_stoi_desc* d) {
  if (stoi_check(d) != CTN_OK) return 0;
  return (size_t)STOI_TAB_FILTER + (d->up == d->down ? 0 : 2 * (size_t)d->Hl + 1);
}

extern "C" size_t ctn_stoi_workspace_bytes(const ctn_stoi_desc* d) {
  if (stoi_check(d) != CTN_OK) return 0;
  return stoi_layout(d->M, d->C, d->E, d->T, d->up, d->down).bytes;
}

extern "C" int ctn_stoi_eval(const ctn_stoi_desc* d, const float* refs, const float* sigs, const int32_t* lengths,
                             const double* tab, double* score, int32_t* kept, int32_t* status, void* ws,
                             size_t ws_bytes, void* stream) {
  if (int rc = stoi_check(d)) return rc;
  if (!refs || !sigs || !lengths || !tab || !score || !kept || !status) return fail(CTN_ERR_ARG, "null pointer");
  StoiArgs a{};
  a.M = d->M; a.C = d->C; a.E = d->E; a.T = d->T; a.up = d->up; a.down = d->down; a.Hl = d->Hl;
  a.L = stoi_layout(d->M, d->C, d->E, d->T, d->up, d->down);
  if (!ws || ws_bytes < a.L.bytes) return fail(CTN_ERR_WORKSPACE, "workspace %zu < %zu", ws_bytes, a.L.bytes);
  a.refs = refs; a.sigs = sigs; a.lengths = lengths; a.tab = tab;
  a.score = score; a.kept = kept; a.status = status;
  a.ws = reinterpret_cast<char*>(ws);
  CTN_HIP(launch_stoi_eval(a, (hipStream_t)stream));
  return CTN_OK;
}
