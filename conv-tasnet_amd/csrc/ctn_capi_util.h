// Helpers shared by the C-ABI files (ctn_capi_*.hip): the error buffer behind
// ctn_last_error, the kernel timer's scope, the device error word, and workspace carving.
// The state itself (error buffer, g_timer, the __device__ error word) is defined once, in
// ctn_capi_core.hip.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "../../include/ctn.h"
#include "ctn_common.h"
#include "ctn_kernels.h"

namespace ctn {

// formats the calling thread's ctn_last_error text and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define CTN_HIP(expr)                                                               \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) return fail(CTN_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
  } while (0)

constexpr double kEps = 1e-8;   // conv_tasnet.py:10

// ---------------------------------------------------------------------------
// kernel timer (bench.py roofline measurement): a set of kernel kinds (CTN_TIMER_*), each
// launch of a selected kind bracketed by a pair of hipEvents on the launch's stream
// ---------------------------------------------------------------------------
struct Timer {
  std::mutex mu;
  uint32_t mask = 0;
  int cap = 0;                              // launches per kind
  int stride = 1;                           // bracket every stride-th launch of a kind
  int used[32] = {};
  long seen[32] = {};                       // launches of a kind since enable
  std::vector<hipEvent_t> ev[32];           // pairs
};
extern Timer g_timer;

struct TimedScope {
  hipStream_t s;
  int kind = 0, idx = -1;
  TimedScope(int k, hipStream_t st) : s(st), kind(k) {
    if (k <= 0 || k >= 32 || !((g_timer.mask >> k) & 1u)) return;
    std::lock_guard<std::mutex> lk(g_timer.mu);
    if (g_timer.seen[k]++ % g_timer.stride != 0 || g_timer.used[k] >= g_timer.cap) return;
    idx = g_timer.used[k]++;
    (void)hipEventRecord(g_timer.ev[k][2 * idx], s);
  }
  ~TimedScope() {
    if (idx >= 0) (void)hipEventRecord(g_timer.ev[kind][2 * idx + 1], s);
  }
};

// ---------------------------------------------------------------------------
// device error word (ctn_capi_core.hip)
// ---------------------------------------------------------------------------
// the mirror of earlier copies (no synchronisation): non-zero once an error has been seen
int dev_err_check_async();
// copy the current device's word to its pinned host mirror on stream s
hipError_t dev_err_refresh(hipStream_t s);

// ---------------------------------------------------------------------------
// workspace carving
// ---------------------------------------------------------------------------
struct Carver {
  char* base;
  size_t off = 0;
  explicit Carver(void* b) : base((char*)b) {}
  template <typename P> P* take(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    P* p = base ? reinterpret_cast<P*>(base + off) : nullptr;
    off += bytes;
    return p;
  }
};
inline size_t esize(int dt) { return dt == CTN_DTYPE_BF16 ? 2 : 4; }
// scratch floats of the two-level slab reduction for one (nparts, n) descriptor
inline size_t sr_tmp(long nparts, long n) {
  const long ns = (nparts + 63) / 64;
  return ns > 1 ? (size_t)(ns * n) : 0;
}

}  // namespace ctn
