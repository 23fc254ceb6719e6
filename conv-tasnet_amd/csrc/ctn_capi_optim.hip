// C-ABI entries of parameter update and weight packing (include/ctn.h ctn_opt_*, ctn_adam_*, ctn_pack_weights).
#include "ctn_capi_util.h"

using namespace ctn;

// ===========================================================================
// Parameter update (clip_grad_norm_ + Adam), ctn_optim.hip
// ===========================================================================
static_assert(sizeof(ctn_opt_segment) == sizeof(OptSegment), "segment layout");
static_assert(sizeof(ctn_opt_chunk) == sizeof(OptChunk), "chunk layout");

extern "C" int ctn_opt_plan(const ctn_opt_segment* segs, int nseg, ctn_opt_chunk* chunks, int max_chunks) {
  if (!segs || nseg < 0) return -fail(CTN_ERR_ARG, "ctn_opt_plan: bad segment table");
  long total = 0;
  for (int i = 0; i < nseg; ++i) {
    const ctn_opt_segment& g = segs[i];
    if (g.numel < 0 || !g.grad) return -fail(CTN_ERR_ARG, "ctn_opt_plan: segment %d has no grad or numel < 0", i);
    const uintptr_t ptrs[4] = {(uintptr_t)g.param, (uintptr_t)g.grad, (uintptr_t)g.exp_avg, (uintptr_t)g.exp_avg_sq};
    bool aligned = true;
    for (uintptr_t q : ptrs) aligned = aligned && (q % 16 == 0);
    for (int64_t off = 0; off < g.numel; off += OPT_CHUNK) {
      const int64_t len = g.numel - off < OPT_CHUNK ? g.numel - off : OPT_CHUNK;
      if (chunks && total < max_chunks)
        chunks[total] = ctn_opt_chunk{i, (uint32_t)len | (aligned ? 0u : OPT_UNALIGNED), off};
      ++total;
    }
  }
  if (total > INT32_MAX) return -fail(CTN_ERR_ARG, "ctn_opt_plan: too many chunks");
  return (int)total;
}

extern "C" int ctn_grad_clip_norm(const ctn_opt_segment* segs, const ctn_opt_chunk* chunks, int nchunks,
                                  float max_norm, float* total_norm, float* partial, void* stream) {
  if (!segs || !chunks || !partial || nchunks < 0) return fail(CTN_ERR_ARG, "ctn_grad_clip_norm: null table");
  const hipStream_t s = (hipStream_t)stream;
  const OptSegment* sg = reinterpret_cast<const OptSegment*>(segs);
  const OptChunk* ch = reinterpret_cast<const OptChunk*>(chunks);
  CTN_HIP(launch_grad_sqnorm(sg, ch, nchunks, partial, s));
  CTN_HIP(launch_grad_clip(sg, ch, nchunks, partial, max_norm, total_norm, s));
  return CTN_OK;
}

extern "C" int ctn_adam_step(const ctn_opt_segment* segs, const ctn_opt_chunk* chunks, int nchunks,
                             const ctn_adam_hparams* hp, void* stream) {
  if (!segs || !chunks || !hp || nchunks < 0 || hp->step < 1)
    return fail(CTN_ERR_ARG, "ctn_adam_step: bad arguments");
  // bias corrections of step hp->step in fp64 on the device (adam_bias, ctn_optim.hip)
  AdamArgs a{hp->beta1, hp->beta2, hp->eps, hp->weight_decay, hp->lr, hp->step, nullptr, nullptr};
  CTN_HIP(launch_adam(reinterpret_cast<const OptSegment*>(segs), reinterpret_cast<const OptChunk*>(chunks), nchunks,
                      a, (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_opt_write_segments(ctn_opt_segment* dst, const ctn_opt_segment* src, int n, void* stream) {
  if (!dst || n < 0 || (n > 0 && !src)) return fail(CTN_ERR_ARG, "ctn_opt_write_segments: bad arguments");
  CTN_HIP(launch_write_segments(reinterpret_cast<OptSegment*>(dst), reinterpret_cast<const OptSegment*>(src), n,
                                (hipStream_t)stream));
  return CTN_OK;
}

extern "C" int ctn_adam_step_dev(const ctn_opt_segment* segs, const ctn_opt_chunk* chunks, int nchunks,
                                 const ctn_adam_hparams* hp, const float* lr_dev, int32_t* counter, void* stream) {
  if (!segs || !chunks || !hp || nchunks < 0 || !counter)
    return fail(CTN_ERR_ARG, "ctn_adam_step_dev: bad arguments");
  AdamArgs a{hp->beta1, hp->beta2, hp->eps, hp->weight_decay, hp->lr, 1, lr_dev, nullptr};
  CTN_HIP(launch_adam_dev(reinterpret_cast<const OptSegment*>(segs), reinterpret_cast<const OptChunk*>(chunks),
                          nchunks, a, counter, (hipStream_t)stream));
  return CTN_OK;
}

// ===========================================================================
// Weight packing (bf16 compute copies for a whole step)
// ===========================================================================
static_assert(sizeof(ctn_weight_pack) == sizeof(PrepDesc), "pack layout");

extern "C" int ctn_pack_weights(const ctn_weight_pack* packs, int n, void* stream) {
  if (n < 0 || (n > 0 && !packs)) return fail(CTN_ERR_ARG, "ctn_pack_weights: bad table");
  for (int i = 0; i < n; ++i) {
    const ctn_weight_pack& w = packs[i];
    if (!w.src || w.rows <= 0 || w.cols <= 0 || (!w.dst && !w.dst_t && !w.dst_frag && !w.dst_t_frag))
      return fail(CTN_ERR_ARG, "ctn_pack_weights: entry %d is empty or has no destination", i);
    if ((w.dst_frag || w.dst_t_frag) && (w.rows % 32 || w.cols % 32))
      return fail(CTN_ERR_ARG, "ctn_pack_weights: entry %d: fragment order needs rows and cols in multiples of 32 "
                  "(%d x %d)", i, w.rows, w.cols);
  }
  for (int i0 = 0; i0 < n; i0 += PREP_MAX) {
    PrepBatch pb{};
    pb.nd = n - i0 < PREP_MAX ? n - i0 : PREP_MAX;
    for (int i = 0; i < pb.nd; ++i) {
      const ctn_weight_pack& w = packs[i0 + i];
      pb.d[i] = PrepDesc{w.src, w.rows, w.cols, w.dst, w.dst_t, w.dst_frag, w.dst_t_frag};
    }
    CTN_HIP(launch_prep_weights(BF16, pb, (hipStream_t)stream));
  }
  return CTN_OK;
}
