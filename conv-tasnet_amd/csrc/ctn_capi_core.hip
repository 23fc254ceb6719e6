// extern "C" entry points of libctn_hip.so (include/ctn.h) and the native launch
// sequences behind them live in the ctn_capi_*.hip files, one per family.  Each entry
// validates its descriptor, carves the caller's workspace, and enqueues its kernels on the
// caller's stream.  This file: ABI version, error string, kernel timers, the device error
// word, and the copy / MFMA-peak entries; it defines the state the families share
// (ctn_capi_util.h).
#include <stdarg.h>

#include <atomic>

#include "ctn_capi_util.h"

using namespace ctn;

static thread_local char g_err[512] = "";

int ctn::fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" int ctn_abi_version(void) { return CTN_ABI_VERSION; }
extern "C" const char* ctn_last_error(void) { return g_err; }
extern "C" int ctn_padded_frames(int K) { return ((K + 127) / 128) * 128; }

// ---------------------------------------------------------------------------
// kernel timer (Timer, TimedScope: ctn_capi_util.h)
// ---------------------------------------------------------------------------
Timer ctn::g_timer;

extern "C" int ctn_timer_enable_mask(uint32_t mask, int max_launches) {
  if (max_launches < 0 || (mask & 1u)) return fail(CTN_ERR_ARG, "timer mask 0x%x / launches %d", mask, max_launches);
  std::lock_guard<std::mutex> lk(g_timer.mu);
  for (int k = 0; k < 32; ++k) {
    for (auto e : g_timer.ev[k]) (void)hipEventDestroy(e);
    g_timer.ev[k].clear();
    g_timer.used[k] = 0;
    g_timer.seen[k] = 0;
  }
  g_timer.mask = max_launches ? mask : 0u;
  g_timer.cap = max_launches;
  for (int k = 1; k < 32; ++k) {
    if (!((g_timer.mask >> k) & 1u)) continue;
    g_timer.ev[k].resize(2 * (size_t)g_timer.cap);
    for (auto& e : g_timer.ev[k]) CTN_HIP(hipEventCreate(&e));
  }
  return CTN_OK;
}

extern "C" int ctn_timer_set_stride(int stride) {
  if (stride < 1) return fail(CTN_ERR_ARG, "timer stride %d", stride);
  std::lock_guard<std::mutex> lk(g_timer.mu);
  g_timer.stride = stride;
  return CTN_OK;
}

extern "C" int ctn_copy_bytes(void* dst, const void* src, size_t bytes, int workgroups, int flags, void* stream) {
  if (!dst || !src || bytes % 16 || ((uintptr_t)dst | (uintptr_t)src) % 16 || workgroups < 1 ||
      workgroups > 65536 || (flags & ~3))
    return fail(CTN_ERR_ARG, "copy: %zu bytes, %d workgroups, flags %d (16-byte multiples and alignment, 1..65536, "
                "flags 0..3)", bytes, workgroups, flags);
  CTN_HIP(ctn::launch_copy_stream(dst, src, bytes, workgroups, flags, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_mfma_peak(int shape, int workgroups, int iters, float* out, double* flops, void* stream) {
  if (!out || workgroups < 1 || workgroups > 65536 || iters < 1 || (shape != 0 && shape != 1))
    return fail(CTN_ERR_ARG, "mfma_peak: shape %d, %d workgroups, %d iterations (shape 0|1, 1..65536, >= 1)", shape,
                workgroups, iters);
  CTN_HIP(ctn::launch_mfma_peak(shape, workgroups, iters, out, flops, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_timer_enable(int kind, int max_launches) {
  if (kind < 0 || kind >= 32) return fail(CTN_ERR_ARG, "timer kind %d", kind);
  return ctn_timer_enable_mask(kind ? 1u << kind : 0u, kind ? max_launches : 0);
}

extern "C" int ctn_timer_read_kind(int kind, double* total_ms, int* launches) {
  if (kind <= 0 || kind >= 32) return fail(CTN_ERR_ARG, "timer kind %d", kind);
  std::lock_guard<std::mutex> lk(g_timer.mu);
  double t = 0.0;
  for (int i = 0; i < g_timer.used[kind]; ++i) {
    CTN_HIP(hipEventSynchronize(g_timer.ev[kind][2 * i + 1]));
    float ms = 0.f;
    CTN_HIP(hipEventElapsedTime(&ms, g_timer.ev[kind][2 * i], g_timer.ev[kind][2 * i + 1]));
    t += ms;
  }
  if (total_ms) *total_ms = t;
  if (launches) *launches = g_timer.used[kind];
  return CTN_OK;
}

extern "C" int ctn_timer_read(double* total_ms, int* launches) {
  double t = 0.0;
  int n = 0;
  for (int k = 1; k < 32; ++k) {
    double tk = 0.0;
    int nk = 0;
    const int rc = ctn_timer_read_kind(k, &tk, &nk);
    if (rc) return rc;
    t += tk;
    n += nk;
  }
  if (total_ms) *total_ms = t;
  if (launches) *launches = n;
  return CTN_OK;
}

// ---------------------------------------------------------------------------
// device error word (ctn_common.h CTN_DEVERR_*): one per device, a zero-initialised
// __device__ variable of this code object (each device loads its own copy), so getting it
// needs no allocation and no memset: safe on the first launch even inside a stream or
// graph capture.  The pointer is cached per device in an atomic, so launches take no lock.
// A pinned host mirror is refreshed asynchronously at the end of every backward pass
// (ctn_tblock_reduce_grads) and checked at the next one, so a kernel that hit an error
// fails the call within a step without a device synchronisation on the fast path.
// ---------------------------------------------------------------------------
__device__ uint32_t ctn_err_words[64];   // [0] is the word; the rest pads it to its own line

namespace {
constexpr int MAX_DEV = 64;
struct DevErr {
  std::mutex mu;
  std::atomic<uint32_t*> word[MAX_DEV] = {};
  std::atomic<uint32_t*> mirror[MAX_DEV] = {};
};
DevErr g_deverr;

uint32_t* dev_err_word(int* dev) {
  if (hipGetDevice(dev) != hipSuccess || *dev < 0 || *dev >= MAX_DEV) return nullptr;
  uint32_t* w = g_deverr.word[*dev].load(std::memory_order_acquire);
  if (w) return w;
  void* a = nullptr;
  if (hipGetSymbolAddress(&a, HIP_SYMBOL(ctn_err_words)) != hipSuccess) return nullptr;
  g_deverr.word[*dev].store((uint32_t*)a, std::memory_order_release);
  return (uint32_t*)a;
}

// the pinned host mirror of a device's word (allocated on the first refresh or status
// call, never on a kernel launch)
volatile uint32_t* dev_err_mirror(int dev) {
  uint32_t* h = g_deverr.mirror[dev].load(std::memory_order_acquire);
  if (h) return h;
  std::lock_guard<std::mutex> lk(g_deverr.mu);
  h = g_deverr.mirror[dev].load(std::memory_order_relaxed);
  if (!h) {
    void* p = nullptr;
    if (hipHostMalloc(&p, 256, hipHostMallocDefault) != hipSuccess) return nullptr;
    *(volatile uint32_t*)p = 0u;
    h = (uint32_t*)p;
    g_deverr.mirror[dev].store(h, std::memory_order_release);
  }
  return h;
}

const char* dev_err_text(uint32_t w) {
  if (w & CTN_DEVERR_SPIN)
    return "a generation-word wait of a wave-specialised kernel ran out of polls (CTN_DEVERR_SPIN): that launch's "
           "outputs are invalid";
  return "unknown device error bit";
}
}  // namespace

int ctn::dev_err_check_async() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return CTN_OK;
  const uint32_t* h = g_deverr.mirror[dev].load(std::memory_order_acquire);
  if (!h) return CTN_OK;
  const uint32_t w = *(const volatile uint32_t*)h;
  if (w) return fail(CTN_ERR_HIP, "device error word 0x%x: %s", w, dev_err_text(w));
  return CTN_OK;
}

hipError_t ctn::dev_err_refresh(hipStream_t s) {
  int dev = 0;
  uint32_t* w = dev_err_word(&dev);
  volatile uint32_t* h = w ? dev_err_mirror(dev) : nullptr;
  if (!h) return hipErrorOutOfMemory;
  return hipMemcpyAsync((void*)h, w, 4, hipMemcpyDeviceToHost, s);
}

uint32_t* ctn::device_error_word() {
  int dev = 0;
  return dev_err_word(&dev);
}

extern "C" int ctn_device_status(void* stream, uint32_t* word, int clear) {
  int dev = 0;
  uint32_t* dw = dev_err_word(&dev);
  volatile uint32_t* mirror = dw ? dev_err_mirror(dev) : nullptr;
  if (!mirror) return fail(CTN_ERR_HIP, "device error word: unavailable");
  hipStream_t s = (hipStream_t)stream;
  uint32_t w = 0;
  CTN_HIP(hipStreamSynchronize(s));
  CTN_HIP(hipMemcpy(&w, dw, 4, hipMemcpyDeviceToHost));
  if (clear && w) {
    CTN_HIP(hipMemset(dw, 0, 4));
    *mirror = 0u;
  }
  if (word) *word = w;
  if (w) return fail(CTN_ERR_HIP, "device error word 0x%x: %s", w, dev_err_text(w));
  return CTN_OK;
}
