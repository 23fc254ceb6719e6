// C-ABI entries of streaming causal separation and its graph cache (include/ctn.h ctn_stream_*).
#include "ctn_capi_util.h"

using namespace ctn;

// ===========================================================================
// Streaming causal separation (ctn_stream.hip)
// ===========================================================================
namespace {
int stream_check(const ctn_stream_desc* d) {
  if (!d) return fail(CTN_ERR_ARG, "null descriptor");
  if (d->M < 1 || d->K < 1) return fail(CTN_ERR_ARG, "M=%d K=%d", d->M, d->K);
  if (d->L < 2 || d->L % 2 || d->L > 64) return fail(CTN_ERR_UNSUPPORTED, "L=%d (even, <= 64)", d->L);
  if (d->N < 1 || d->B < 1 || d->H < 1 || d->P < 1 || d->P > 8 || d->C < 1 || d->C > 8)
    return fail(CTN_ERR_ARG, "N=%d B=%d H=%d P=%d C=%d", d->N, d->B, d->H, d->P, d->C);
  if (d->norm != CTN_NORM_CLN && d->norm != CTN_NORM_BN)
    return fail(CTN_ERR_UNSUPPORTED, "norm %d: gLN normalizes over the whole utterance and cannot stream", d->norm);
  if (d->mask_type < 0 || d->mask_type > 2) return fail(CTN_ERR_ARG, "mask type %d", d->mask_type);
  return CTN_OK;
}
StreamArgs stream_args(const ctn_stream_desc* d) {
  StreamArgs a{};
  a.M = d->M; a.K = d->K; a.N = d->N; a.L = d->L; a.B = d->B; a.H = d->H; a.P = d->P; a.C = d->C;
  a.norm = d->norm == CTN_NORM_CLN ? 1 : 2;
  a.mask_type = d->mask_type;
  return a;
}
}  // namespace

extern "C" int ctn_stream_encode(const ctn_stream_desc* d, const float* samples, int64_t ld_samples, const float* U,
                                 const float* gamma0, const float* beta0, const float* wb_t, float* w_out,
                                 float* x_out, void* stream) {
  if (int rc = stream_check(d)) return rc;
  if (!samples || !U || !gamma0 || !beta0 || !wb_t || !w_out || !x_out) return fail(CTN_ERR_ARG, "null pointer");
  if (ld_samples < (int64_t)(d->K - 1) * (d->L / 2) + d->L) return fail(CTN_ERR_ARG, "ld_samples too small");
  StreamArgs a = stream_args(d);
  a.samples = samples; a.ld_samples = ld_samples; a.U = U; a.na = gamma0; a.nb = beta0; a.W = wb_t;
  a.w_out = w_out; a.x_out = x_out;
  CTN_HIP(launch_stream(0, a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_stream_block(const ctn_stream_desc* d, int dilation, int64_t pos, int ring_frames,
                                const float* x_in, const float* w1_t, const float* alpha1, const float* norm1_a,
                                const float* norm1_b, const float* wd, const float* alpha2, const float* norm2_a,
                                const float* norm2_b, const float* w2_t, float* ring, float* x_out, void* stream) {
  if (int rc = stream_check(d)) return rc;
  if (dilation < 1 || pos < 0) return fail(CTN_ERR_ARG, "dilation %d, pos %lld", dilation, (long long)pos);
  if (ring_frames < 1 || (ring_frames & (ring_frames - 1)) || ring_frames < (d->P - 1) * dilation + d->K)
    return fail(CTN_ERR_ARG, "ring_frames %d: a power of two >= (P-1)*dilation + K = %d", ring_frames,
                (d->P - 1) * dilation + d->K);
  if (!x_in || !w1_t || !alpha1 || !norm1_a || !norm1_b || !wd || !alpha2 || !norm2_a || !norm2_b || !w2_t || !ring ||
      !x_out)
    return fail(CTN_ERR_ARG, "null pointer");
  if (x_in == x_out) return fail(CTN_ERR_ARG, "x_out must not alias x_in (the residual is read per frame)");
  StreamArgs a = stream_args(d);
  a.dil = dilation; a.pos = pos; a.R = ring_frames; a.x_in = x_in; a.ring = ring;
  a.W = w1_t; a.alpha1 = alpha1; a.na = norm1_a; a.nb = norm1_b;
  CTN_HIP(launch_stream(1, a, (hipStream_t)stream));
  a.W = w2_t; a.alpha2 = alpha2; a.na = norm2_a; a.nb = norm2_b; a.wd = wd; a.x_out = x_out;
  CTN_HIP(launch_stream(2, a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_stream_decode(const ctn_stream_desc* d, const float* x_last, const float* w, const float* wm_t,
                                 const float* V, const float* tail_in, float* tail_out, float* frames_ws, float* out,
                                 void* stream) {
  if (int rc = stream_check(d)) return rc;
  if (!x_last || !w || !wm_t || !V || !tail_in || !tail_out || !frames_ws || !out) return fail(CTN_ERR_ARG, "null pointer");
  if (tail_in == tail_out) return fail(CTN_ERR_ARG, "tail_out must not alias tail_in");
  StreamArgs a = stream_args(d);
  a.x_in = x_last; a.w_in = w; a.W = wm_t; a.V = V; a.tail_in = tail_in; a.tail_out = tail_out;
  a.frames = frames_ws; a.out = out;
  CTN_HIP(launch_stream(3, a, (hipStream_t)stream));
  return CTN_OK;
}

// ABI v7: one whole streaming call (ctn_stream.hip, launch_stream_call_stage)
namespace {
size_t stream_ws_floats(const ctn_stream_desc* d) {
  const size_t M = d->M, K = d->K;
  return M * K * d->N + 2 * M * K * d->B + M * K * (size_t)(d->H > d->C * d->N ? d->H : d->C * d->N);
}
// the replayed graph's pos slot: 16-byte aligned, inside the workspace's 256-byte tail
long* stream_pos_slot(const ctn_stream_desc* d, void* ws) {
  const size_t off = (stream_ws_floats(d) * sizeof(float) + 15) / 16 * 16;
  return reinterpret_cast<long*>(reinterpret_cast<char*>(ws) + off);
}
// CTN_STREAM_GRAPH=0: launch the stages directly on every call (A/B only)
bool stream_graph_enabled() {
  const char* e = getenv("CTN_STREAM_GRAPH");
  return e ? atoi(e) != 0 : true;
}
struct StreamGraph {
  std::vector<uintptr_t> key;
  hipGraphExec_t exec;
  hipEvent_t done;   // recorded after every launch of exec (launches of one exec are ordered)
};
std::mutex g_sg_mu;
std::vector<StreamGraph> g_sg;   // most recently stored last; at most 8
// Finds (or builds with `build`) the graph of `key` and launches it on s behind a
// pos store, all under the cache lock, so no other thread can evict the graph between
// the lookup and the launch.  An evicted graph is destroyed after the lock is released,
// once its own last launch has finished (its event): no device-wide synchronisation,
// nothing that would stall other streams or invalidate another thread's capture.
template <typename Build>
hipError_t stream_graph_launch(const std::vector<uintptr_t>& key, Build build, long* pos_dev, long pos, hipStream_t s) {
  StreamGraph victim{{}, nullptr, nullptr};
  hipError_t e = hipSuccess;
  {
    std::lock_guard<std::mutex> lk(g_sg_mu);
    StreamGraph* g = nullptr;
    for (StreamGraph& x : g_sg)
      if (x.key == key) g = &x;
    if (!g) {
      hipGraphExec_t exec = nullptr;
      hipEvent_t ev = nullptr;
      e = build(&exec);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) {
        if (exec) (void)hipGraphExecDestroy(exec);
        return e;
      }
      if (g_sg.size() == 8) {
        victim = g_sg.front();
        g_sg.erase(g_sg.begin());
      }
      g_sg.push_back(StreamGraph{key, exec, ev});
      g = &g_sg.back();
    }
    e = launch_stream_set_pos(pos_dev, pos, s);
    if (e == hipSuccess) e = hipGraphLaunch(g->exec, s);
    if (e == hipSuccess) e = hipEventRecord(g->done, s);
  }
  if (victim.exec) {   // a ninth distinct argument set (rare)
    (void)hipEventSynchronize(victim.done);
    (void)hipGraphExecDestroy(victim.exec);
    (void)hipEventDestroy(victim.done);
  }
  return e;
}
}  // namespace

extern "C" size_t ctn_stream_workspace_bytes(const ctn_stream_desc* d) {
  if (stream_check(d)) return 0;
  return stream_ws_floats(d) * sizeof(float) + 256;
}

extern "C" int ctn_stream_call(const ctn_stream_desc* d, const ctn_stream_model* mdl, int64_t pos, const float* samples,
                               int64_t ld_samples, const float* tail_in, float* tail_out, float* out, void* ws,
                               size_t ws_bytes, void* stream) {
  if (int rc = stream_check(d)) return rc;
  if (!mdl || !samples || !tail_in || !tail_out || !out || !ws) return fail(CTN_ERR_ARG, "null pointer");
  if (!mdl->U || !mdl->gamma0 || !mdl->beta0 || !mdl->wb_t || !mdl->wm_t || !mdl->V || (mdl->nblocks && !mdl->blocks))
    return fail(CTN_ERR_ARG, "null model pointer");
  if (mdl->nblocks < 0) return fail(CTN_ERR_ARG, "nblocks %d", mdl->nblocks);
  if (pos < 0) return fail(CTN_ERR_ARG, "pos %lld", (long long)pos);
  if (tail_in == tail_out) return fail(CTN_ERR_ARG, "tail_out must not alias tail_in");
  if (ld_samples < (int64_t)(d->K - 1) * (d->L / 2) + d->L) return fail(CTN_ERR_ARG, "ld_samples too small");
  if (ws_bytes < ctn_stream_workspace_bytes(d)) return fail(CTN_ERR_WORKSPACE, "workspace too small");
  for (int i = 0; i < mdl->nblocks; ++i) {
    const ctn_stream_block_params& b = mdl->blocks[i];
    if (b.dilation < 1 || b.ring_frames < 1 || (b.ring_frames & (b.ring_frames - 1)) ||
        b.ring_frames < (d->P - 1) * b.dilation + d->K)
      return fail(CTN_ERR_ARG, "block %d: dilation %d, ring_frames %d (a power of two >= (P-1)*dilation + K)", i,
                  b.dilation, b.ring_frames);
    if (!b.w1_t || !b.alpha1 || !b.norm1_a || !b.norm1_b || !b.wd || !b.alpha2 || !b.norm2_a || !b.norm2_b ||
        !b.w2_t || !b.ring)
      return fail(CTN_ERR_ARG, "block %d: null pointer", i);
  }
  const hipStream_t s = (hipStream_t)stream;
  long* pos_dev = stream_pos_slot(d, ws);
  // the launch sequence, parameterised by where `pos` comes from
  auto enqueue = [&](hipStream_t q, const long* pd) -> hipError_t {
    const size_t M = d->M, K = d->K;
    float* w = reinterpret_cast<float*>(ws);
    float* xa = w + M * K * d->N;
    float* xb = xa + M * K * d->B;
    float* scratch = xb + M * K * d->B;   // h1 of a block / the sources
    StreamArgs a = stream_args(d);
    a.pos = pos; a.pos_dev = pd;
    a.samples = samples; a.ld_samples = ld_samples; a.U = mdl->U; a.na = mdl->gamma0; a.nb = mdl->beta0;
    a.W = mdl->wb_t; a.w_out = w; a.x_out = xa;
    hipError_t e = launch_stream_call_stage(0, a, q);
    float* x = xa;
    float* y = xb;
    for (int i = 0; e == hipSuccess && i < mdl->nblocks; ++i) {
      const ctn_stream_block_params& b = mdl->blocks[i];
      StreamArgs ab = stream_args(d);
      ab.pos = pos; ab.pos_dev = pd; ab.dil = b.dilation; ab.R = b.ring_frames; ab.ring = b.ring;
      ab.x_in = x; ab.x_out = y; ab.frames = scratch;
      ab.W = b.w1_t; ab.alpha1 = b.alpha1; ab.na = b.norm1_a; ab.nb = b.norm1_b;
      ab.wd = b.wd; ab.alpha2 = b.alpha2; ab.na2 = b.norm2_a; ab.nb2 = b.norm2_b; ab.W2 = b.w2_t;
      e = launch_stream_call_stage(1, ab, q);
      if (e == hipSuccess) e = launch_stream_call_stage(2, ab, q);
      float* t = x; x = y; y = t;
    }
    StreamArgs ad = stream_args(d);
    ad.x_in = x; ad.w_in = w; ad.W = mdl->wm_t; ad.V = mdl->V; ad.frames = scratch;
    ad.tail_in = tail_in; ad.tail_out = tail_out; ad.out = out;
    if (e == hipSuccess) e = launch_stream_call_stage(3, ad, q);
    if (e == hipSuccess) e = launch_stream_call_stage(4, ad, q);
    return e;
  };
  if (!stream_graph_enabled()) {
    CTN_HIP(enqueue(s, nullptr));
    return CTN_OK;
  }
  // Graph replay: the 4 + 2 X R launches of a call are captured once per argument set
  // (everything but pos, which the replay reads from the workspace) and replayed with
  // one graph launch after a one-thread kernel stores pos.
  std::vector<uintptr_t> key;
  int dev = 0;
  CTN_HIP(hipGetDevice(&dev));
  key.push_back((uintptr_t)dev);
  for (const int v : {d->M, d->K, d->N, d->L, d->B, d->H, d->P, d->C, d->norm, d->mask_type}) key.push_back((uintptr_t)(unsigned)v);
  for (const void* v : {(const void*)mdl->U, (const void*)mdl->gamma0, (const void*)mdl->beta0, (const void*)mdl->wb_t,
                        (const void*)mdl->wm_t, (const void*)mdl->V, (const void*)samples, (const void*)tail_in,
                        (const void*)tail_out, (const void*)out, (const void*)ws})
    key.push_back((uintptr_t)v);
  key.push_back((uintptr_t)ld_samples);
  {   // a forced chunk width (ctn_stream.hip, sc_width) picks other kernels: another graph
    const char* e = getenv("CTN_SC_W");
    key.push_back((uintptr_t)(e ? (atoi(e) == 8 ? 8 : 32) : 0));
  }
  for (int i = 0; i < mdl->nblocks; ++i) {
    const ctn_stream_block_params& b = mdl->blocks[i];
    key.push_back((uintptr_t)(unsigned)b.dilation);
    key.push_back((uintptr_t)(unsigned)b.ring_frames);
    for (const void* v : {(const void*)b.w1_t, (const void*)b.alpha1, (const void*)b.norm1_a, (const void*)b.norm1_b,
                          (const void*)b.wd, (const void*)b.alpha2, (const void*)b.norm2_a, (const void*)b.norm2_b,
                          (const void*)b.w2_t, (const void*)b.ring})
      key.push_back((uintptr_t)v);
  }
  auto build = [&](hipGraphExec_t* exec) -> hipError_t {
    hipStream_t cs = nullptr;
    hipError_t e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    hipGraph_t g = nullptr;
    e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
      const hipError_t el = enqueue(cs, pos_dev);
      e = hipStreamEndCapture(cs, &g);
      if (el != hipSuccess) e = el;
    }
    if (e == hipSuccess) e = hipGraphInstantiate(exec, g, nullptr, nullptr, 0);
    if (g) (void)hipGraphDestroy(g);
    (void)hipStreamDestroy(cs);
    return e;
  };
  CTN_HIP(stream_graph_launch(key, build, pos_dev, (long)pos, s));
  return CTN_OK;
}
