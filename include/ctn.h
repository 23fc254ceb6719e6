/*
 * ctn.h — C ABI of libctn_hip.so, the MI355X (gfx950) Conv-TasNet hot path.
 *
 * Plain C: device pointers, sizes, a HIP stream passed as void*.  No torch
 * types.  The library never allocates: every scratch buffer is a caller-owned
 * workspace sized by the matching *_workspace_bytes() query, and every output
 * buffer is caller-owned.  Functions are reentrant (no global mutable state
 * except the opt-in kernel timer) and run on the caller's current device.
 * Return value: CTN_OK (0) or a ctn_status error code; ctn_last_error()
 * returns a static description of the last error on the calling thread.
 *
 * Layout convention: frame-major row tensors [M*Kp][C] with
 * channels contiguous, Kp = frames padded to a multiple of 128 per utterance
 * (ctn_padded_frames()); padded rows are zero.  Parameters are fp32 in the
 * reference's own shapes ([out,in,1] conv weights etc.); gradients are
 * written (not accumulated) as fp32 in the same shapes.
 *
 * Each entry names the reference interface it replaces (jwr1995/Conv-TasNet,
 * src/ paths).  The reference binds no FFI: its boundary is the torch.nn.Module
 * API of src/conv_tasnet.py (imported as `from conv_tasnet import ConvTasNet`,
 * src/train.py:12) plus `from pit_criterion import cal_loss`
 * (src/solver.py:9).  The Python drop-in in conv-tasnet_amd/ binds these
 * entries through ctypes.
 */
#ifndef CTN_H
#define CTN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CTN_ABI_VERSION 13

typedef enum { CTN_DTYPE_F32 = 0, CTN_DTYPE_BF16 = 1 } ctn_dtype;
/* CTN_NORM_BN: torch.nn.BatchNorm1d, chose_norm's fallback branch (conv_tasnet.py:302-303) */
typedef enum { CTN_NORM_GLN = 0, CTN_NORM_CLN = 1, CTN_NORM_BN = 2 } ctn_norm_type;
typedef enum { CTN_MASK_RELU = 0, CTN_MASK_SOFTMAX = 1 } ctn_mask_type;
typedef enum {
  CTN_OK = 0,
  CTN_ERR_ARG = 1,          /* invalid argument / shape */
  CTN_ERR_UNSUPPORTED = 2,  /* valid for the reference, not implemented here */
  CTN_ERR_WORKSPACE = 3,    /* workspace smaller than *_workspace_bytes() */
  CTN_ERR_HIP = 4           /* a HIP runtime call failed */
} ctn_status;

int ctn_abi_version(void);
const char* ctn_last_error(void);
/* frames padded to the row-tile multiple used by every kernel (128) */
int ctn_padded_frames(int K);

/* -------------------------------------------------------------------------
 * TemporalBlock: x + DSConv(norm(PReLU(Conv1x1_{B->H}(x))))
 * replaces TemporalBlock.forward, src/conv_tasnet.py:212-238, with
 * DepthwiseSeparableConv :241-272, Chomp1d :275-289, chose_norm :292-303,
 * ChannelwiseLayerNorm :307-329, GlobalLayerNorm :332-355, nn.PReLU :218,253.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t M, K, Kp;         /* utterances, frames, padded frames */
  int32_t B, H, P;          /* bottleneck ch., block ch., depthwise kernel size */
  int32_t dilation;         /* 2**x, conv_tasnet.py:175 */
  int32_t causal;           /* 0/1, conv_tasnet.py:176 */
  int32_t norm_type;        /* ctn_norm_type */
  int32_t dtype;            /* ctn_dtype of activations (and MFMA inputs) */
} ctn_tblock_desc;

typedef struct {            /* fp32 device pointers, reference shapes */
  const float* w1;          /* [H,B,1] net.0.weight */
  const float* alpha1;      /* [1]     net.1.weight */
  const float* gamma1;      /* [1,H,1] net.2.gamma */
  const float* beta1;       /* [1,H,1] net.2.beta */
  const float* wd;          /* [H,1,P] net.3.net.0.weight */
  const float* alpha2;      /* [1]     net.3.net.{1|2}.weight */
  const float* gamma2;      /* [1,H,1] net.3.net.{2|3}.gamma */
  const float* beta2;       /* [1,H,1] net.3.net.{2|3}.beta */
  const float* w2;          /* [B,H,1] net.3.net.{3|4}.weight */
  /* optional bf16 compute copies made by ctn_pack_weights (dtype BF16 only; NULL:
   * the call converts w1/w2 itself): W1 [H][B], W2 [B][H] and their transposes */
  const void* w1_bf16;
  const void* w2_bf16;
  const void* w1t_bf16;     /* [B][H] */
  const void* w2t_bf16;     /* [H][B] */
  /* norm_type CTN_NORM_BN only (gamma/beta above = BatchNorm1d weight/bias, [H]):
   * running statistics of net.2 and net.3.net.{2|3} (NULL: none, batch statistics
   * always), updated in place by a training-mode forward with the unbiased batch
   * variance; `bn_momentum` is torch's exponential factor (momentum, or
   * 1/num_batches_tracked when momentum is None) */
  float* bn_mean1;
  float* bn_var1;
  float* bn_mean2;
  float* bn_var2;
  int32_t bn_training;      /* 1: batch statistics (train mode), 0: running statistics */
  float bn_momentum1, bn_momentum2;
  float bn_eps1, bn_eps2;
  /* optional (ABI v6, dtype BF16, B and H multiples of 32): the same four bf16 copies in
   * MFMA fragment order (ctn_weight_pack dst_frag / dst_t_frag), from which the
   * weight-stationary kernels load their resident weight 1 KiB contiguous per wave;
   * NULL: they read the row-major copies above */
  const void* w1_frag;
  const void* w2_frag;
  const void* w1t_frag;
  const void* w2t_frag;
} ctn_tblock_params;

/* One fp32 weight [rows][cols] -> bf16 copy (dst, same layout) and/or bf16
 * transpose (dst_t, [cols][rows]), and (ABI v6) the same two in MFMA fragment order
 * (dst_frag, dst_t_frag; rows and cols multiples of 32): element (n, k) of a [O][I]
 * matrix at ((g*2 + nb)*(I/32) + kb)*512 + lane*8 + e for n = g*32 + ((lane&15)>>2)*8
 * + nb*4 + (lane&3), k = kb*32 + (lane>>4)*8 + e.  Any destination may be NULL. */
typedef struct {
  const float* src;
  int32_t rows, cols;
  void* dst;
  void* dst_t;
  void* dst_frag;
  void* dst_t_frag;
} ctn_weight_pack;
/* Converts n weights in ceil(n / 64) launches (a training step's bf16 weight
 * copies for all TemporalBlocks at once, instead of per block call). */
int ctn_pack_weights(const ctn_weight_pack* packs, int n, void* stream);

typedef struct {            /* fp32 outputs, same shapes as ctn_tblock_params */
  float *w1, *alpha1, *gamma1, *beta1, *wd, *alpha2, *gamma2, *beta2, *w2;
} ctn_tblock_grads;

typedef struct {            /* forward results kept for backward */
  void* h1;                 /* [M*Kp, H] pre-PReLU output of the first 1x1 conv */
  void* d;                  /* [M*Kp, H] pre-PReLU output of the depthwise conv */
  float* stats;             /* [4*G]: (mean,rstd) of norm1 then norm2; G = M (gLN), M*Kp (cLN) or H (BN) */
} ctn_tblock_saved;

int ctn_tblock_stats_floats(const ctn_tblock_desc* d);
size_t ctn_tblock_workspace_bytes(const ctn_tblock_desc* d, int backward);
int ctn_tblock_forward(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x, void* y,
                       const ctn_tblock_saved* saved, void* ws, size_t ws_bytes, void* stream);
int ctn_tblock_backward(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                        const ctn_tblock_saved* saved, const void* gy, void* gx,
                        const ctn_tblock_grads* g, void* ws, size_t ws_bytes, void* stream);
/* ABI v6: the same backward with its parameter-gradient tail on a second stream.  The
 * data-gradient chain (gx) is queued on `stream`; the first 1x1 conv's weight-gradient
 * GEMM and all parameter-gradient reductions wait for an event recorded on `stream`
 * once their inputs exist and run on `wgrad_stream`, so they overlap the previous
 * block's backward on `stream`.  The caller keeps x, ws and the gradient outputs alive
 * and unmodified until `wgrad_stream` has finished this call's work, and orders the
 * consumers of g after it (norm_type BN: everything on `stream`). */
int ctn_tblock_backward_split(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                              const ctn_tblock_saved* saved, const void* gy, void* gx,
                              const ctn_tblock_grads* g, void* ws, size_t ws_bytes, void* stream,
                              void* wgrad_stream);

/* ABI v8: the same backward with every parameter-gradient reduction left for later, so
 * that one call can reduce all blocks of a backward pass (a few launches instead of two
 * per block).  The fixed-order partial sums go to `part` (ctn_tblock_partials_bytes(d)
 * bytes; ws then needs only ctn_tblock_deferred_workspace_bytes(d)); the gradients in
 * `g` are NOT written by this call.  gLN / cLN blocks only (BN: CTN_ERR_UNSUPPORTED).
 * Replaces, for a whole backward pass, the per-block gradient writes of the reference's
 * TemporalBlock backward (src/conv_tasnet.py:217-263, autograd).                       */
size_t ctn_tblock_partials_bytes(const ctn_tblock_desc* d);
size_t ctn_tblock_deferred_workspace_bytes(const ctn_tblock_desc* d);
int ctn_tblock_backward_deferred(const ctn_tblock_desc* d, const ctn_tblock_params* p, const void* x,
                                 const ctn_tblock_saved* saved, const void* gy, void* gx,
                                 const ctn_tblock_grads* g, void* ws, size_t ws_bytes, void* part,
                                 size_t part_bytes, void* stream);
/* Write the gradients g[i] of n deferred block backwards from their partials parts[i]
 * (each part[i] unmodified since its ctn_tblock_backward_deferred call; descs[i] the same
 * descriptor).  Bit-identical to the per-block reductions of ctn_tblock_backward.       */
int ctn_tblock_reduce_grads(const ctn_tblock_desc* descs, const ctn_tblock_grads* g, void* const* parts, int n,
                            void* stream);

/* -------------------------------------------------------------------------
 * Front of the network: Encoder (src/conv_tasnet.py:97-117: ReLU(Conv1d(1,N,L,
 * stride L/2))) + the TemporalConvNet input cLN (:167, :307-329) + bottleneck
 * 1x1 conv N->B (:169).  wb == NULL: encoder only (standalone Encoder).
 * Back of the network: mask 1x1 conv B->C*N (:185), mask nonlinearity
 * (:202-208), Decoder (:120-142), overlap_and_add (src/utils.py:9-46) and the
 * F.pad to T (:56-59).  wm == NULL: standalone Decoder, `x_last` then holds
 * the mask rows [M*Kp, C*N] and mask_type must be CTN_MASK_IDENTITY.
 * ------------------------------------------------------------------------- */
#define CTN_MASK_IDENTITY 2
typedef struct {
  int32_t M, T, K, Kp;      /* utterances, samples, frames = (T-L)/(L/2)+1, padded frames */
  int32_t N, L, B, C;       /* encoder filters, filter length, bottleneck ch., speakers */
  int32_t mask_type;        /* ctn_mask_type or CTN_MASK_IDENTITY */
  int32_t dtype;            /* ctn_dtype of activations */
} ctn_codec_desc;

size_t ctn_encoder_workspace_bytes(const ctn_codec_desc* d, int backward);
int ctn_encoder_forward(const ctn_codec_desc* d, const float* mixture, const float* U, const float* gamma0,
                        const float* beta0, const float* wb, void* w_rows, float* cln_stats, void* x0,
                        void* ws, size_t ws_bytes, void* stream);
int ctn_encoder_backward(const ctn_codec_desc* d, const float* mixture, const float* U, const float* gamma0,
                         const float* beta0, const float* wb, const void* w_rows, const float* cln_stats,
                         const void* g_w_rows, const void* g_x0, float* gU, float* ggamma0, float* gbeta0,
                         float* gwb, void* ws, size_t ws_bytes, void* stream);

size_t ctn_decoder_workspace_bytes(const ctn_codec_desc* d, int backward);
int ctn_decoder_forward(const ctn_codec_desc* d, const void* x_last, const void* w_rows, const float* wm,
                        const float* V, void* score, float* est, void* ws, size_t ws_bytes, void* stream);
int ctn_decoder_backward(const ctn_codec_desc* d, const void* x_last, const void* w_rows, const float* wm,
                         const float* V, const void* score, const float* g_est, void* g_x_last, void* g_w_rows,
                         float* gwm, float* gV, void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * PIT SI-SNR loss: replaces cal_loss / cal_si_snr_with_pit / reorder_source /
 * get_mask, src/pit_criterion.py:12-113.  `est` is masked in place beyond
 * each length (:37-38); `reordered` (nullable) keeps the reference's
 * perm-not-inverse indexing (:91-97).  `coef` [M*C*4] is saved for backward.
 * 1 <= C <= 16 (0 workspace bytes / CTN_ERR_UNSUPPORTED beyond): C <= 10 searches all C!
 * permutations (:66) and keeps the first maximum (torch.argmax); 11 <= C <= 16, past what
 * the reference's C!-row one-hot table can hold, solves the same maximum as a linear
 * assignment (Hungarian, fp64) and reports its lexicographic rank in best_perm (exact ties
 * may pick another optimal permutation).  The backward is one fp32 pass
 * scale (al s + be e + off), so its relative accuracy degrades in proportion to the
 * estimate's offset / amplitude (8e-6 of a row's largest gradient at offset 100,
 * amplitude 1; 3e-7 at offset 0.3).  The encoder/decoder descriptors accept 1..16
 * (streaming: 1..8).
 * ------------------------------------------------------------------------- */
typedef struct { int32_t M, C, T; } ctn_pit_desc;
size_t ctn_pit_workspace_bytes(const ctn_pit_desc* d);
int ctn_pit_forward(const ctn_pit_desc* d, const float* source, float* est, const int64_t* lengths, float* loss,
                    float* max_snr, int64_t* best_perm, float* reordered, float* coef, void* ws, size_t ws_bytes,
                    void* stream);
int ctn_pit_backward(const ctn_pit_desc* d, const float* source, const float* est, const int64_t* lengths,
                     const float* coef, const float* g_loss, const float* g_max_snr, float* g_est, void* stream);

/* -------------------------------------------------------------------------
 * MixIT loss (mixture-invariant training, Wisdom et al. 2020): the model separates a
 * mixture of two recordings into C outputs; every output is assigned to one of the two
 * recordings, and the two remixed sums are scored against the recordings under the best
 * assignment.  Added within ABI v13 without a version bump (nothing existing changed):
 * callers probe for the symbol.  No reference counterpart (src/pit_criterion.py needs
 * isolated sources); DESIGN.md §27 has the full definition.
 *
 * mixtures [M][2][T], est [M][C][T] fp32 contiguous, 2 <= C <= 8, lengths [M] (>= 1; values
 * above T count as T).  All sums run over t < lengths[m]; nothing is masked in place.
 * Assignment p in [0, 2^C): bit c of p is the recording of output c; y_n = sum of the outputs
 * with bit n (an empty set gives 0).  EPS = 1e-8.
 *   mode CTN_MIXIT_SNR:    snr_n = 10 log10((X_n + EPS) / (R_n + tau X_n + EPS)), X_n = sum x_n^2,
 *                          R_n = sum (x_n - y_n)^2, tau = 10^(-snr_max / 10);
 *   mode CTN_MIXIT_SI_SNR: the SI-SNR of ctn_pit_forward on (y_n, x_n), both with their own
 *                          mean over t < length removed; snr_max is not read.
 * max_snr[m] = max_p (snr_0 + snr_1) / 2, the first maximum in ascending p -> assign[m];
 * loss = -mean_m max_snr[m]; remix [M][2][T] (nullable) = y_n under assign[m], added in fp32
 * in ascending c, zero at t >= length.  All statistics and the search are fp64 in a fixed
 * order without atomics: two calls on the same inputs give the same bits.  coef [M][2][4]
 * (al, be, off, unused) is saved for the backward,
 *   g_est[m][c][t] = (g_max_snr[m] - g_loss / M) (al_n x_n[t] + be_n y_n[t] + off_n), n = bit c
 * of assign[m], for t < length and exactly 0 beyond (g_max_snr nullable: zeros).
 * An unsupported descriptor (C < 2, C > 8, unknown mode, non-finite snr_max) has 0 workspace
 * bytes; the entries check descriptor, pointers and workspace before anything is launched,
 * and neither synchronises (both can be captured into a graph).
 * ------------------------------------------------------------------------- */
enum { CTN_MIXIT_SNR = 0, CTN_MIXIT_SI_SNR = 1 };
typedef struct { int32_t M, C, T, mode; float snr_max; } ctn_mixit_desc;
size_t ctn_mixit_workspace_bytes(const ctn_mixit_desc* d);
int ctn_mixit_forward(const ctn_mixit_desc* d, const float* mixtures, const float* est, const int64_t* lengths,
                      float* loss, float* max_snr /*[M]*/, int64_t* assign /*[M]*/, float* remix /*[M][2][T]*/,
                      float* coef /*[M][2][4]*/, void* ws, size_t ws_bytes, void* stream);
int ctn_mixit_backward(const ctn_mixit_desc* d, const float* mixtures, const float* est, const int64_t* lengths,
                       const int64_t* assign, const float* coef, const float* g_loss, const float* g_max_snr,
                       float* g_est /*[M][C][T]*/, void* stream);

/* -------------------------------------------------------------------------
 * PIT with silent sources (Wisdom et al. 2021, "What's all the FUSS about free universal sound
 * separation data?", section 4): a model with C outputs is scored against 0 ... C speaking
 * references.  An active reference is scored by (SI-)SNR, a silent one by how far its output
 * lies below the mixture, and the permutation is searched over both kinds together.  Added
 * within ABI v13 without a version bump (nothing existing changed): callers probe for the
 * symbol.  No reference counterpart; DESIGN.md §29 has the full definition.
 *
 * source, est [M][C][T], mixture [M][T] (nullable) fp32 contiguous, 2 <= C <= 8, lengths [M]
 * (>= 1; values above T count as T).  All sums run over t < n = min(lengths[m], T) in fp64;
 * nothing is masked in place and est is never written.  EPS = 1e-8, tau = 10^(-snr_max / 10),
 * tau0 = 10^(-inactive_snr_max / 10).
 *   x = mixture, or without one x[t] = sum_j s_j[t] in ascending j;  X = sum x^2.
 *   Reference j is active iff S_j = sum s_j^2 > 0: inactive iff every sample inside the length
 *   is +-0 (no threshold).  active [M][C] receives 1 / 0.
 *   Output i against an active j:
 *     mode CTN_PITVAR_SNR:    10 log10((S_j + EPS) / (R_ij + tau S_j + EPS)), R_ij = sum (s_j - e_i)^2;
 *     mode CTN_PITVAR_SI_SNR: the zero-mean SI-SNR of ctn_pit_forward, both means over t < n.
 *   Output i against an inactive j: 10 log10((X + EPS) / (E_i + tau0 X + EPS)), E_i = sum e_i^2.
 * perm [M][C] (perm[m][i] = the reference of output i) maximises sum_i score[i][perm[i]] over
 * all C! permutations: the first maximum in lexicographic (itertools.permutations) order, which
 * decides the k! exact ties of k silent references.  max_snr[m] = that sum / C;
 * loss = -mean_m max_snr[m].  All statistics and the search are fp64 in a fixed order without
 * atomics: two calls on the same inputs give the same bits.  coef [M][C][4] (al, be, off, j) is
 * saved for the backward,
 *   g_est[m][i][t] = (g_max_snr[m] - g_loss / M) (al s_j[t] + be e_i[t] + off),
 * for t < n and exactly 0 beyond (g_max_snr nullable: zeros); al = 0 for an inactive j.
 * An unsupported descriptor (C < 2, C > 8, unknown mode, non-finite snr_max or
 * inactive_snr_max) has 0 workspace bytes; the entries check descriptor, pointers and workspace
 * before anything is launched, and neither synchronises (both can be captured into a graph).
 * ------------------------------------------------------------------------- */
enum { CTN_PITVAR_SNR = 0, CTN_PITVAR_SI_SNR = 1 };
typedef struct { int32_t M, C, T, mode; float snr_max, inactive_snr_max; } ctn_pitvar_desc;
size_t ctn_pitvar_workspace_bytes(const ctn_pitvar_desc* d);
int ctn_pitvar_forward(const ctn_pitvar_desc* d, const float* source, const float* est, const float* mixture,
                       const int64_t* lengths, float* loss, float* max_snr /*[M]*/, int64_t* perm /*[M][C]*/,
                       uint8_t* active /*[M][C]*/, float* coef /*[M][C][4]*/, void* ws, size_t ws_bytes,
                       void* stream);
int ctn_pitvar_backward(const ctn_pitvar_desc* d, const float* source, const float* est, const int64_t* lengths,
                        const float* coef, const float* g_loss, const float* g_max_snr,
                        float* g_est /*[M][C][T]*/, void* stream);

/* -------------------------------------------------------------------------
 * Mixture-consistency projection (Wisdom et al. 2019, "Differentiable consistency
 * constraints for improved deep speech enhancement"): the residual of the model's C outputs
 * against the input mixture is spread over the outputs, so that they add up to the mixture.
 * Added within ABI v13 without a version bump (nothing existing changed): callers probe for
 * the symbol.  No reference counterpart; DESIGN.md §28 has the full definition.
 *
 * mixture [M][T], est [M][C][T] fp32 contiguous, 2 <= C <= 16, lengths [M] int64 or null
 * (= T); n = min(max(lengths[m], 0), T).  EPS = 1e-8.  For t < n
 *   r[t] = x[t] - sum_j s_j[t] (ascending j),  out_c[t] = s_c[t] + w_c r[t],
 * evaluated in fp64 per sample and rounded to fp32 once; for t >= n out_c[t] = s_c[t] bit for
 * bit.  Not in place (out != est).
 *   mode CTN_MIXCON_UNIFORM: w_c = 1 / C; coef is not touched (nullable).
 *   mode CTN_MIXCON_POWER:   p_c = sum_{t<n} s_c[t]^2, D = sum_c p_c + C EPS,
 *                            w_c = (p_c + EPS) / D; coef [M][C+1] fp64 receives w_c and D and
 *                            is what the backward reads.
 * Backward, g_out = dL/d out:  G[t] = sum_c w_c g_c[t],
 *   g_est_k[t] = g_k[t] - G[t] + 2 s_k[t] (a_k - sum_c w_c a_c) / D,  a_c = sum_{t<n} g_c[t] r[t]
 * (the third term in power mode only), g_mixture[t] = G[t] (nullable: not written); for
 * t >= n g_est = g_out bit for bit and g_mixture = 0.  fp64 per sample, rounded once.  In
 * uniform mode the backward reads neither mixture, est nor coef (all nullable).
 * All sums are fp64 in a fixed order without atomics: two calls on the same inputs give the
 * same bits.  One workspace size serves both directions.  An unsupported descriptor
 * (C < 2, C > 16, M or T < 1, unknown mode) has 0 workspace bytes; the entries check
 * descriptor, pointers and workspace before anything is launched, and neither synchronises
 * (both can be captured into a graph).
 * ------------------------------------------------------------------------- */
enum { CTN_MIXCON_UNIFORM = 0, CTN_MIXCON_POWER = 1 };
typedef struct { int32_t M, C, T, mode; } ctn_mixcon_desc;
size_t ctn_mixcon_workspace_bytes(const ctn_mixcon_desc* d);
int ctn_mixcon_forward(const ctn_mixcon_desc* d, const float* mixture, const float* est, const int64_t* lengths,
                       float* out /*[M][C][T]*/, double* coef /*[M][C+1]*/, void* ws, size_t ws_bytes, void* stream);
int ctn_mixcon_backward(const ctn_mixcon_desc* d, const float* mixture, const float* est, const int64_t* lengths,
                        const double* coef, const float* g_out, float* g_est /*[M][C][T]*/,
                        float* g_mixture /*[M][T]*/, void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * BSS Eval v3 source metrics (ABI v13): the energies behind the SDR / SIR / SAR of
 * mir_eval.separation.bss_eval_sources, which src/evaluate.py:90-105 calls on the host
 * once per utterance.  For M utterances, C references and E scored signals per utterance,
 * each signal is decomposed against the references with `flen`-tap distortion filters
 * (the normal equations of the lag correlations, factored once per utterance and system
 * and solved for all E signals).  fp32 inputs with row stride T samples; utterance m uses
 * its first lengths[m] samples and never reads the rest (it may hold NaN).  All arithmetic
 * is fp64 in a fixed order: two calls on the same inputs give the same bits.
 * energies[m][e][j] = { |s_true+e_spat|^2, |e_interf|^2, |e_interf+e_artif|^2,
 *                       |s_true+e_spat+e_interf|^2, |e_artif|^2 } of signal e against
 * reference j: SDR = 10 log10(v0/v2), SIR = 10 log10(v0/v1), SAR = 10 log10(v3/v4).
 * status[m] = 1 when a Cholesky pivot of one of utterance m's systems was not finite or
 * <= order * 2^-52 * (largest diagonal entry) (rank-deficient references: its energies are
 * then meaningless), else 0.  Limits: C * flen <= 4096, T >= flen, M and E <= 65535
 * (0 workspace bytes / an error code beyond).
 * ------------------------------------------------------------------------- */
typedef struct { int32_t M, C, E, T, flen; } ctn_bss_desc;   /* T = row stride in samples */
size_t ctn_bss_workspace_bytes(const ctn_bss_desc* d);
int ctn_bss_eval(const ctn_bss_desc* d, const float* refs /*[M][C][T]*/, const float* sigs /*[M][E][T]*/,
                 const int32_t* lengths /*[M]*/, double* energies /*[M][E][C][5]*/, int32_t* status /*[M]*/,
                 void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * STOI and ESTOI (short-time objective intelligibility: Taal et al., IEEE TASLP 19(7), 2011;
 * Jensen & Taal, IEEE TASLP 24(11), 2016) as pystoi 0.3+ computes them, for M utterances,
 * C references and E scored signals per utterance: score[m][e][j] = { STOI, ESTOI } of
 * signal e against reference j.  Added within ABI v13 without a version bump (nothing
 * existing changed): callers probe for the symbol.  fp32 inputs with row stride T samples;
 * utterance m uses its first lengths[m] samples and never reads the rest (it may hold NaN).
 *
 * `tab` (device memory, ctn_stoi_table_doubles(d) doubles, computed by the caller in fp64;
 * the kernels evaluate no trigonometric function):
 *   [0, 256)    the window w = hanning(258)[1:-1];
 *   [256, 768)  the twiddles, cos(2 pi k / 512) at 256 + 2 k and -sin(2 pi k / 512) at
 *               256 + 2 k + 1, k < 256;
 *   [768, ...)  hh = up * win, 2 Hl + 1 taps with hh[-Hl] first, win the unit-sum low-pass
 *               of the resampler (stoi.resample_filter); absent for 1/1.
 *
 * Stages, all fp64, every sum in a fixed order, no atomics (two calls on the same inputs
 * give the same bits; a row's result does not depend on the other rows of the batch):
 *  1. resampling to 10 kHz by the reduced ratio up/down = 10000 / rate:
 *     r[k] = sum_i hh[k down - i up + Hl] s[i], k < n10 = ceil(length up / down), i ascending
 *     over the samples inside the signal, acc = acc + hh s without FMA contraction (the index
 *     formula of ctn_dmix_mix_sp); 1/1 copies exactly;
 *  2. frames k < K = (n10 - 256) / 128 + 1 (0 for n10 < 256) of a reference,
 *     nrm_k = |w r[128 k : 128 k + 256]|_2; frame k is kept iff
 *     (nrm_k + EPS) * 100 > max_k nrm_k + EPS (EPS = 2^-52), i.e. less than 40 dB below the
 *     loudest; idx[0 ... kept - 1] are the kept frame numbers, kept[m][j] their count.  The
 *     mask of reference j is applied to reference j and to every signal scored against it;
 *  3. frame j < kept of the overlap-add z of the kept windowed frames at hop 128, rebuilt
 *     from the kept frames idx[j-1], idx[j], idx[j+1] added in that order (z is not stored),
 *     windowed again, zero-padded to 512; reference and signal as x + i y through one complex
 *     FFT, split by conjugate symmetry (a frame of all zeros has exactly zero envelopes,
 *     not the other signal's rounding residue); X[b][j], Y[b][j] = sqrt(sum of |.|^2 over the bins
 *     [lo_b, hi_b)) of the 15 third-octave bands from 150 Hz, lo = 7 9 11 14 17 22 27 34 43 55
 *     69 87 109 138 174, hi = lo shifted by one band, then 219;
 *  4. segments s < J = kept - 29 of 30 frames.  STOI: per band, ys scaled by
 *     |xs| / (|ys| + EPS), clipped at xs (1 + 10^(15/20)), both mean-subtracted and divided by
 *     (norm + EPS), their inner products summed over bands and segments and divided by 15 J.
 *     ESTOI: xs and ys mean-subtracted and divided by (norm + EPS) along the frames, then the
 *     same along the bands; sum of (xn yn / 30) divided by J;
 *  5. kept[m][j] < 30: both scores are 1e-5 (pystoi's value) and status[m][j] = 1, else 0.
 * The call allocates nothing and does not synchronise the host; everything runs on `stream`.
 * Limits: 1 <= M, E <= 65535; 1 <= C <= 16; T >= 1; 1 <= up, down <= 64 and reduced;
 * 1 <= Hl <= 4096 unless up = down = 1 (Hl is then ignored); ceil(T up / down) < 2^31;
 * lengths in [1, T] (a length outside [0, T] is clamped into it on the device).  Beyond a
 * limit: 0 doubles / 0 workspace bytes / an error code with a ctn_last_error message;
 * arguments are validated before any device access.
 * ------------------------------------------------------------------------- */
typedef struct { int32_t M, C, E, T;   /* T = row stride in samples */
                 int32_t up, down, Hl; } ctn_stoi_desc;
size_t ctn_stoi_table_doubles(const ctn_stoi_desc* d);   /* 256 + 512 + (up == down ? 0 : 2 Hl + 1) */
size_t ctn_stoi_workspace_bytes(const ctn_stoi_desc* d);
int ctn_stoi_eval(const ctn_stoi_desc* d, const float* refs /*[M][C][T]*/, const float* sigs /*[M][E][T]*/,
                  const int32_t* lengths /*[M]*/, const double* tab,
                  double* score /*[M][E][C][2]: STOI, ESTOI*/, int32_t* kept /*[M][C]*/,
                  int32_t* status /*[M][C]: 1 = fewer than 30 kept frames, score = 1e-5*/,
                  void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * Dynamic mixing: training batches drawn and mixed on the device from a resident corpus
 * of single-speaker utterances, instead of the host collation of fixed mixtures
 * (src/data.py:131-159 _collate_fn, :237-271 load_mixtures_and_sources).  Added within ABI v13
 * without a version bump (nothing existing changed): callers probe for the symbol.
 * Corpus (caller-owned device memory): `pool`, all utterances back to back — pool_dtype 0:
 * int16 PCM, a sample s has the value s * 2^-15; 1: fp32 —, `off` [n_utts + 1] sample
 * offsets, `spk` [n_utts] speaker ids, `elig` [n_elig] the utterances of at least T samples.
 *
 * ctn_dmix_draw fills plan[M][C].  Row m is global sample g = first_sample + m; the random
 * words of slot c, try j are Philox4x32-10 with counter (g_lo, g_hi, c, j) and key
 * (seed_lo, seed_hi): utt = elig[(r0 * n_elig) >> 32], start = (r1 * (len - T + 1)) >> 32,
 * level_db = lo + (hi - lo) * (r2 >> 8) * 2^-24 (fp32).  Slots are drawn in order; a
 * candidate whose speaker equals an accepted earlier slot's is rejected and j advances;
 * after max_tries candidates the last one is kept; `tries` = candidates drawn.  A row
 * depends on (seed, g) only.  An elig entry outside [0, n_utts), or naming an utterance
 * shorter than T or of 2^31 samples or more, gives utt = -1 (which ctn_dmix_mix flags).
 * first_sample_dev != NULL: g is read from that device word (first_sample is ignored) and a
 * second kernel then adds `advance` to it, so that a captured launch replays correctly.
 *
 * ctn_dmix_mix takes a plan (drawn, or written by the caller).  Gain of (m, c) before the
 * guard: level_mode 0: 10^(level_db / 20); 1: 10^(level_db / 20) / max(rms, 1e-4), rms over
 * the segment's T samples (fp64, per-chunk partial sums finished in index order).  peak > 0:
 * p = max_t |sum_c fl32(g_c x_c)|; if p > peak every gain of the row becomes
 * fl32(g_c * fl32(peak / p)).  gains[m][c] is the gain applied;
 * sources[m][c][t] = fl32(gains[m][c] * x) (x exact, one rounding); mixture[m][t] = the fp32
 * sum of the stored sources added left to right from c = 0; no FMA contraction anywhere.
 * An entry with utt outside [0, n_utts), start < 0 or start + T > len is never
 * dereferenced: its row (sources, mixture, gains) is written as zeros and status[m] = 1,
 * else status[m] = 0.  No atomics; every sum and max has a fixed order.
 * Limits: M >= 1, 1 <= C <= 16, T >= 1, n_utts >= 1, n_elig >= 1, 1 <= max_tries <= 64,
 * pool_dtype and level_mode 0 or 1, finite levels and peak (0 workspace bytes / an error
 * code beyond).
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t M, C, T;          /* rows, slots (speakers) per row, samples per segment */
  int32_t n_utts, n_elig;
  int32_t pool_dtype;       /* 0 int16 PCM, 1 fp32 */
  int32_t level_mode;       /* 0 gain from level_db alone, 1 relative to the segment RMS */
  int32_t max_tries;
  float level_lo_db, level_hi_db;
  float peak;               /* 0: no peak guard */
  uint64_t seed;
} ctn_dmix_desc;
typedef struct { int32_t utt, start; float level_db; int32_t tries; } ctn_dmix_entry;
size_t ctn_dmix_workspace_bytes(const ctn_dmix_desc* d);
int ctn_dmix_draw(const ctn_dmix_desc* d, const int64_t* off /*[n_utts+1]*/, const int32_t* spk /*[n_utts]*/,
                  const int32_t* elig /*[n_elig]*/, int64_t first_sample, int64_t* first_sample_dev,
                  int64_t advance, ctn_dmix_entry* plan /*[M][C]*/, void* stream);
int ctn_dmix_mix(const ctn_dmix_desc* d, const void* pool, const int64_t* off /*[n_utts+1]*/,
                 const ctn_dmix_entry* plan /*[M][C]*/, float* gains /*[M][C]*/, float* sources /*[M][C][T]*/,
                 float* mixture /*[M][T]*/, int32_t* status /*[M]*/, void* ws, size_t ws_bytes, void* stream);

/* Dynamic mixing with a drawn number of speakers: after any of the draw entries, row m keeps
 * n_m = min_speakers + ((r0 (C - min_speakers + 1)) >> 32) of its C slots, r0 = word 0 of
 * philox4x32_10((g_lo, g_hi, 48, 0), seed) for the row's global sample g (a counter word 2 next
 * to the RIR draws' 16 + c and the noise draw's 32: no existing draw moves).  Slots c >= n_m get
 * level_db = -inf, every other bit of the plan stays; count[m] = n_m.  The mix entries need no
 * change: exp10(-inf / 20) is exactly 0 in both level modes, so a thinned slot drops out of the
 * mixture, the peak guard and the noise power, and its written source is +-0 everywhere.
 * g = (first_sample_dev ? *first_sample_dev - drawn_advance : first_sample) + m: pass the draw's
 * `advance` as drawn_advance when the draw moved the device counter.  1 <= min_speakers <= C
 * (CTN_ERR_ARG beyond); min_speakers = C keeps every slot.  Added within ABI v13 without a
 * version bump (nothing existing changed): callers probe for the symbol.  DESIGN.md §29. */
int ctn_dmix_thin(const ctn_dmix_desc* d, int32_t min_speakers, int64_t first_sample,
                  const int64_t* first_sample_dev, int64_t drawn_advance, ctn_dmix_entry* plan /*[M][C]*/,
                  int32_t* count /*[M]*/, void* stream);

/* -------------------------------------------------------------------------
 * Dynamic mixing with speed perturbation: every source is resampled by a polyphase FIR
 * before it is mixed, so that it plays at e.g. 95, 100 or 105 % speed (pitch and tempo
 * change).  Added like dynamic mixing itself, without an ABI bump: callers probe for the
 * symbol.  ctn_dmix_draw and ctn_dmix_mix are unchanged.
 *
 * Speed table: n entries, 1 <= n <= 8.  Entry k is a reduced ratio up/down, output rate
 * over input rate; the speed in percent is 100 * down / up (95 % = 20/19, 105 % = 20/21).
 * Limits: 1 <= up, down <= 64, gcd(up, down) = 1, up <= 2 down, down <= 2 up.  1/1 means
 * "no resampling".
 *
 * Filter of an entry (the design of scipy.signal.resample_poly): Hl = 10 * max(up, down),
 * 2 Hl + 1 taps, h[n] = fc sinc(fc n) kaiser(2 Hl + 1, beta = 5.0)[n + Hl] for n = -Hl ... Hl
 * with fc = 1 / max(up, down), normalised to unit sum and multiplied by `up`; computed in
 * fp64 by the caller and rounded once to fp32.  `filt` (device memory) holds the filters
 * of the entries back to back, h[-Hl] first, none for a 1/1 entry:
 * ctn_dmix_sp_filter_floats(speeds) floats.  The kernel evaluates no transcendental.
 *
 * Resampled segment of a slot (utt, start, speed k): with x[i] = utt[start + i] as the
 * exact fp32 value (s * 2^-15 for PCM16) and x[i] = 0 for start + i outside [0, len),
 *   xr[n] = sum_i h[n down - i up + Hl] x[i],  n = 0 ... T - 1,
 * i running upward from ceil((n down - Hl) / up) to floor((n down + Hl) / up), each step
 * acc = fl32(acc + fl32(h x)) from acc = 0, no FMA contraction, int64 index arithmetic.
 * Terms whose x lies outside the utterance are skipped and never read (the neighbouring
 * utterance of the pool does not leak in).  For 1/1, xr[n] = x[n] exactly.
 * span_k = floor((T - 1) down_k / up_k) + 1 input samples lie under the T output centres.
 * A slot is valid when 0 <= k < n, 0 <= utt < n_utts, 0 <= start and
 * start + span_k <= len; the filter's tails may overhang the utterance (those taps
 * contribute zero).  An invalid slot is never dereferenced: its row is zeros and
 * status[m] = 1, as in ctn_dmix_mix.
 *
 * ctn_dmix_draw_sp: the Philox call of ctn_dmix_draw; of each candidate first
 * k = (r3 * n) >> 32, then utt = elig[(r0 * n_elig) >> 32], then
 * start = (r1 * (len - span_k + 1)) >> 32 (utt = -1 when len < span_k); level_db, the
 * speaker rejection, `tries` and the device-counter form are unchanged.  speed[m][c] = k of
 * the kept candidate.  `elig` should hold the utterances of at least max_k span_k samples.
 * With the table {1/1} the plan is that of ctn_dmix_draw.
 *
 * ctn_dmix_mix_sp: resamples every slot into the workspace (xr [M][C][T]) and runs the
 * level, RMS, peak-guard and write stages of ctn_dmix_mix on xr, whose contract composes:
 * sources[m][c][t] = fl32(gains[m][c] * xr), the mixture summed left to right.  With every
 * slot at 1/1 the outputs are those of ctn_dmix_mix.  Beyond the limits: 0 floats / 0
 * workspace bytes / an error code.
 * ------------------------------------------------------------------------- */
typedef struct { int32_t n; struct { int32_t up, down; } r[8]; } ctn_dmix_speeds;
size_t ctn_dmix_sp_filter_floats(const ctn_dmix_speeds* speeds);   /* sum of 2 Hl_k + 1; 1/1 entries 0 */
size_t ctn_dmix_sp_workspace_bytes(const ctn_dmix_desc* d, const ctn_dmix_speeds* speeds);
int ctn_dmix_draw_sp(const ctn_dmix_desc* d, const ctn_dmix_speeds* speeds, const int64_t* off /*[n_utts+1]*/,
                     const int32_t* spk /*[n_utts]*/, const int32_t* elig /*[n_elig]*/, int64_t first_sample,
                     int64_t* first_sample_dev, int64_t advance, ctn_dmix_entry* plan /*[M][C]*/,
                     int32_t* speed /*[M][C]*/, void* stream);
int ctn_dmix_mix_sp(const ctn_dmix_desc* d, const ctn_dmix_speeds* speeds, const float* filt, const void* pool,
                    const int64_t* off /*[n_utts+1]*/, const ctn_dmix_entry* plan /*[M][C]*/,
                    const int32_t* speed /*[M][C]*/, float* gains /*[M][C]*/, float* sources /*[M][C][T]*/,
                    float* mixture /*[M][T]*/, int32_t* status /*[M]*/, void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * Dynamic mixing with reverberation and noise: every source is optionally convolved with a
 * drawn room impulse response (RIR) and the mixture optionally gets a drawn noise segment at
 * a drawn SNR.  Added without an ABI bump: callers probe for the symbol.  ctn_dmix_draw,
 * ctn_dmix_mix, ctn_dmix_draw_sp and ctn_dmix_mix_sp are unchanged, and with n_rirs = 0 and
 * n_noise_utts = 0 the entries below write their bits (speeds == NULL: the plain pair).
 *
 * RIRs (caller-owned device memory): `rir_pool`, fp32 taps of all RIRs back to back, `roff`
 * [n_rirs + 1] int64 tap offsets; rir_max_taps is the longest of them, 1 ... 16384 (a RIR
 * that is empty or longer makes its row invalid).  Noise: a second pool `noise_pool` of
 * noise_dtype 0 (int16 PCM) or 1 (fp32) with `noff` [n_noise_utts + 1] and `nelig`
 * [n_noise_elig], as the speech pool.  n_rirs = 0: no reverberation; n_noise_utts =
 * n_noise_elig = 0: no noise; the arguments of a stage that is off may be NULL and its outputs
 * (nplan, ngain, noise_out; rir is written as -1 when given) are not touched.
 *
 * Row m (global sample g), slot c:
 * 1. xs[n], n = 0 ... T - 1: the segment ctn_dmix_mix reads, or with a speed table the
 *    resampled segment xr of ctn_dmix_mix_sp.
 * 2. rir[m][c] = k >= 0, taps h[0 ... L - 1] = rir_pool[roff[k] ...]:
 *      xv[n] = sum_{j = 0}^{min(n, L - 1)} h[j] xs[n - j],
 *    j running upward, each step acc = fl32(acc + fl32(h[j] xs[n - j])) from +0, no FMA
 *    contraction.  The segment starts from silence: samples before `start` do not feed the
 *    tail.  k = -1: xv = xs exactly.  k outside [-1, n_rirs): the row is invalid (zeros,
 *    status[m] = 1, nothing dereferenced).  A RIR's neighbours in the pool are never read.
 * 3. The gains before the guard are those of ctn_dmix_mix applied to xv (level_mode 1: the
 *    RMS of xv).
 * 4. Noise, nplan[m] = {utt, start, level_db = snr_db, tries}: z[n] the exact fp32 sample,
 *    s[n] the fp32 left-to-right sum of fl32(g_c xv_c[n]), P_s = (1/T) sum (double)s[n]^2,
 *    P_z likewise (fp64 per-chunk partial sums finished in index order),
 *      g_z = fl32(sqrt(P_s / max(P_z, 1e-8)) * 10^(-snr_db / 20))   (fp64, rounded once).
 *    An invalid noise entry (as a source entry: utt, start, start + T > len) makes the row
 *    invalid.
 * 5. peak > 0: p = max_n |fl32(s[n] + fl32(g_z z[n]))|; if p > peak every gain of the row,
 *    g_z included, becomes fl32(g * fl32(peak / p)).
 * 6. gains[m][c], ngain[m] are the gains applied; sources[m][c][n] = fl32(gains xv) (the
 *    reverberant signals that are in the mixture); mixture[m][n] = the fp32 sum of the stored
 *    sources left to right with fl32(ngain z[n]) added last; noise_out [M][T] (or NULL)
 *    receives fl32(ngain z).  Outputs may sit at any 4-byte alignment.
 *
 * ctn_dmix_draw_aug writes plan (and speed, with a table) with the bits of ctn_dmix_draw(_sp)
 * and, same key,
 *   rir[m][c]: counter (g_lo, g_hi, 16 + c, 0); u = fl32(r1 >> 8) * 2^-24;
 *              u < rir_prob (fp32) ? (r0 * n_rirs) >> 32 : -1     (n_rirs = 0: -1)
 *   nplan[m] : counter (g_lo, g_hi, 32, 0); utt = nelig[(r0 * n_noise_elig) >> 32],
 *              start = (r1 * (len - T + 1)) >> 32, snr_db = lo + (hi - lo) * (r2 >> 8) * 2^-24
 *              (fp32), tries = 1; utt = -1 for a bad nelig entry or an utterance shorter than T.
 * The device-counter form works as in ctn_dmix_draw.
 * Limits: those of ctn_dmix_mix(_sp); 0 <= rir_prob <= 1; finite SNRs; with noise C <= 15
 * (0 workspace bytes / an error code beyond).  No atomics; the only transcendentals are in
 * the one-thread-per-row gain kernels.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t n_rirs;           /* 0: no reverberation */
  int32_t rir_max_taps;     /* the longest RIR of the pool, 1 ... 16384 */
  float rir_prob;           /* a slot is reverberated with this probability */
  int32_t n_noise_utts;     /* 0: no noise */
  int32_t n_noise_elig;
  int32_t noise_dtype;      /* 0 int16 PCM, 1 fp32 */
  float snr_lo_db, snr_hi_db;
} ctn_dmix_aug;
size_t ctn_dmix_aug_workspace_bytes(const ctn_dmix_desc* d, const ctn_dmix_speeds* speeds /*or NULL*/,
                                    const ctn_dmix_aug* aug);
int ctn_dmix_draw_aug(const ctn_dmix_desc* d, const ctn_dmix_speeds* speeds /*or NULL*/, const ctn_dmix_aug* aug,
                      const int64_t* off, const int32_t* spk, const int32_t* elig, const int64_t* noff,
                      const int32_t* nelig, int64_t first_sample, int64_t* first_sample_dev, int64_t advance,
                      ctn_dmix_entry* plan /*[M][C]*/, int32_t* speed /*[M][C], with speeds*/,
                      int32_t* rir /*[M][C]*/, ctn_dmix_entry* nplan /*[M], with noise*/, void* stream);
int ctn_dmix_mix_aug(const ctn_dmix_desc* d, const ctn_dmix_speeds* speeds /*or NULL*/, const ctn_dmix_aug* aug,
                     const float* filt, const void* pool, const int64_t* off, const ctn_dmix_entry* plan,
                     const int32_t* speed, const float* rir_pool, const int64_t* roff /*[n_rirs+1]*/,
                     const int32_t* rir /*[M][C]*/, const void* noise_pool, const int64_t* noff,
                     const ctn_dmix_entry* nplan /*[M]*/, float* gains /*[M][C]*/, float* ngain /*[M]*/,
                     float* sources /*[M][C][T]*/, float* mixture /*[M][T]*/, float* noise_out /*[M][T] or NULL*/,
                     int32_t* status /*[M]*/, void* ws, size_t ws_bytes, void* stream);

/* -------------------------------------------------------------------------
 * Windowed separation of a recording of any length: the mixture x[T] is cut
 * into J overlapping windows of W samples (overlap O, hop Hs = W - O), the model separates
 * the windows as a batch, and the per-window outputs P [J][C][W] are joined on the device.
 * Added without an ABI bump: callers probe for the symbol.
 *
 * J = 1 for T <= W, else 1 + ceil((T - W) / Hs); window j holds x[j Hs ... j Hs + W), zeros at
 * and past T.  Limits: 2 <= C <= 8, 1 <= O <= W/2, T >= 1, T and W <= 2^30, and J as above; a
 * violation, a null pointer or a workspace smaller than ctn_stitch_workspace_bytes() is
 * CTN_ERR_ARG (0 workspace bytes), checked before anything is launched.
 *
 * ctn_stitch_frame writes the windows.
 *
 * ctn_stitch_plan, for every boundary j = 1 ... J-1:
 *   S_j[a][b] = sum_{u < O} P[j-1][a][Hs + u] P[j][b][u]   in fp64 (sim[j], row-major), in
 *   this order: chunk ch covers u in [2048 ch, 2048 ch + 2048); its thread t = 0 ... 255 adds,
 *   from +0, the products at u = 2048 ch + 1024 h + 4 t + e for h = 0, 1 and e = 0 ... 3 in turn
 *   (u >= O adds nothing); the 256 thread sums are added as v[l] += v[l + s], s = 32, 16, ..., 1
 *   inside each group of 64, then ((w0 + w1) + w2) + w3 over the four groups; the chunk sums
 *   are added from +0 in index order.
 *   perm[j] = pi_j maximises sum_a S_j[a][pi_j(a)] (added a = 0 upward); the C! permutations
 *   are taken in lexicographic order and a later one wins only when strictly greater.  If an
 *   entry of S_j is not finite, pi_j is the identity and status[j] = 1 (else 0).
 *   sigma[0] = identity, sigma[j][a] = pi_j(sigma[j-1][a]).  Row 0 of sim, perm and status is
 *   zeros, the identity and 0.
 *
 * ctn_stitch_ola: out[a][t], t < T, with j = min(t / Hs, J - 1) and u = t - j Hs:
 *   j >= 1 and u < O:  fl(fl(fl(1 - fade[u]) p) + fl(fade[u] c)),  p = P[j-1][sigma[j-1][a]][Hs + u],
 *                      c = P[j][sigma[j][a]][u]   (fp32, each operation rounded, no contraction)
 *   otherwise       :  P[j][sigma[j][a]][u]
 * A sigma entry outside [0, C) reads channel a.  No atomics anywhere: the same bits every run.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t J;   /* windows */
  int32_t C;   /* speakers */
  int32_t W;   /* window, samples */
  int32_t O;   /* overlap, samples */
  int32_t T;   /* recording, samples */
} ctn_stitch_desc;
size_t ctn_stitch_workspace_bytes(const ctn_stitch_desc* d);
int ctn_stitch_frame(const ctn_stitch_desc* d, const float* x /*[T]*/, float* win /*[J][W]*/, void* stream);
int ctn_stitch_plan(const ctn_stitch_desc* d, const float* P /*[J][C][W]*/, double* sim /*[J][C][C]*/,
                    int32_t* perm /*[J][C]*/, int32_t* sigma /*[J][C]*/, int32_t* status /*[J]*/, void* ws,
                    size_t ws_bytes, void* stream);
int ctn_stitch_ola(const ctn_stitch_desc* d, const float* P /*[J][C][W]*/, const int32_t* sigma /*[J][C]*/,
                   const float* fade /*[O]*/, float* out /*[C][T]*/, void* stream);

/* -------------------------------------------------------------------------
 * Parameter update: replaces torch.nn.utils.clip_grad_norm_(params, max_norm)
 * (src/solver.py:184-185) and torch.optim.Adam(params, lr, weight_decay=l2)
 * (src/train.py:129-133, stepped at src/solver.py:186) with one launch each
 * over ALL parameter tensors.  A segment describes one parameter tensor (fp32
 * device pointers; exp_avg/exp_avg_sq may be NULL for clipping); the chunk
 * table (ctn_opt_plan, host memory, copied to the device by the caller) cuts
 * the segments into workgroup pieces.  Rebuild the plan whenever a pointer or
 * size changes.
 * ------------------------------------------------------------------------- */
typedef struct {
  float* param;
  float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} ctn_opt_segment;
typedef struct { int32_t seg; uint32_t len; int64_t off; } ctn_opt_chunk;
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  int32_t step;   /* 1-based step count after the increment (bias correction) */
} ctn_adam_hparams;

/* segs: host copy of the segment table.  Returns the number of chunks (writes
 * up to max_chunks entries when chunks != NULL), or a negative ctn_status. */
int ctn_opt_plan(const ctn_opt_segment* segs, int nseg, ctn_opt_chunk* chunks, int max_chunks);
/* grads *= min(1, max_norm / (||grads||_2 + 1e-6)); *total_norm = ||grads||_2 (device).
 * segs/chunks: device tables; partial: device scratch of nchunks floats. */
int ctn_grad_clip_norm(const ctn_opt_segment* segs, const ctn_opt_chunk* chunks, int nchunks, float max_norm,
                       float* total_norm, float* partial, void* stream);
/* one Adam step of every segment (param, exp_avg, exp_avg_sq updated in place); the bias
 * corrections of step hp->step are computed on the device in fp64 (ABI v12) */
int ctn_adam_step(const ctn_opt_segment* segs, const ctn_opt_chunk* chunks, int nchunks, const ctn_adam_hparams* hp,
                  void* stream);

/* Graph capture (ABI v10; torch.optim.Adam(capturable=True) semantics, hipGraph / torch
 * CUDA-graph capture of a whole training step).  No call below reads host memory at
 * launch time from the device, so a captured launch replays correctly:
 *  - ctn_opt_write_segments: writes n segment entries to the device table `dst` with
 *    kernels whose arguments carry the entries (no host staging buffer);
 *  - ctn_adam_step_dev (ABI v12): Adam with the step count in device memory: step
 *    t = *counter + 1, then a second kernel increments *counter; lr = *lr_dev when lr_dev
 *    is not NULL (a schedule writes it between replays), else hp->lr.  The bias
 *    corrections lr / (1 - beta1^t) and sqrt(1 - beta2^t) are computed on the device in
 *    fp64 by the same code as ctn_adam_step's (same bits for the same t and lr), with no
 *    step limit (ABI v10-11 read them from a host-built table of 2^20 steps).
 * hp->step is not read by ctn_adam_step_dev. */
int ctn_opt_write_segments(ctn_opt_segment* dst, const ctn_opt_segment* src, int n, void* stream);
int ctn_adam_step_dev(const ctn_opt_segment* segs, const ctn_opt_chunk* chunks, int nchunks,
                      const ctn_adam_hparams* hp, const float* lr_dev, int32_t* counter, void* stream);

/* -------------------------------------------------------------------------
 * Stand-alone separator layers on frame rows [M*Kp][C] (ABI v4): what the fused
 * calls above run inside themselves, exposed for the reference's module
 * forwards called on their own — TemporalConvNet.forward (src/conv_tasnet.py:
 * 192-209), DepthwiseSeparableConv.forward (:265-272), ChannelwiseLayerNorm.
 * forward (:319-329), GlobalLayerNorm.forward (:344-355) — each with its
 * backward.  Gradients are written, not accumulated.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t M, K, Kp;         /* utterances, frames, padded frames */
  int32_t C;                /* channels of the input rows */
  int32_t dtype;            /* ctn_dtype of activations */
} ctn_rows_desc;

/* gLN / cLN (norm_type CTN_NORM_GLN / CTN_NORM_CLN; EPS 1e-8 inside the sqrt,
 * biased variance, conv_tasnet.py:10,327,353); gamma/beta [1,C,1]; stats
 * [G][2] (mean, rstd), G = M (gLN) or M*Kp (cLN), written by forward */
size_t ctn_layernorm_workspace_bytes(const ctn_rows_desc* d, int norm_type, int backward);
int ctn_layernorm_forward(const ctn_rows_desc* d, int norm_type, const void* x, const float* gamma,
                          const float* beta, void* y, float* stats, void* ws, size_t ws_bytes, void* stream);
int ctn_layernorm_backward(const ctn_rows_desc* d, int norm_type, const void* x, const float* gamma,
                           const float* stats, const void* gy, void* gx, float* ggamma, float* gbeta, void* ws,
                           size_t ws_bytes, void* stream);

/* nn.PReLU() with one shared alpha (conv_tasnet.py:218,253); alpha [1] */
size_t ctn_prelu_workspace_bytes(const ctn_rows_desc* d);
int ctn_prelu_forward(const ctn_rows_desc* d, const void* x, const float* alpha, void* y, void* stream);
int ctn_prelu_backward(const ctn_rows_desc* d, const void* x, const float* alpha, const void* gy, void* gx,
                       float* galpha, void* ws, size_t ws_bytes, void* stream);

/* depthwise Conv1d(C, C, P, dilation, groups=C, bias=False) with the reference's
 * padding (conv_tasnet.py:188,262-265) and, causal, its Chomp1d (:275-289);
 * w [C,1,P]; non-causal needs (P-1)*dilation even (output length K) */
size_t ctn_depthwise_workspace_bytes(const ctn_rows_desc* d, int P);
int ctn_depthwise_forward(const ctn_rows_desc* d, int P, int dilation, int causal, const void* x, const float* w,
                          void* y, void* stream);
int ctn_depthwise_backward(const ctn_rows_desc* d, int P, int dilation, int causal, const void* x, const float* w,
                           const void* gy, void* gx, float* gw, void* ws, size_t ws_bytes, void* stream);

/* Conv1d(C, cout, 1, bias=False) (conv_tasnet.py:169,185,215,270); w [cout,C,1];
 * C and cout multiples of 8 */
size_t ctn_conv1x1_workspace_bytes(const ctn_rows_desc* d, int cout, int backward);
int ctn_conv1x1_forward(const ctn_rows_desc* d, int cout, const void* x, const float* w, void* y, void* ws,
                        size_t ws_bytes, void* stream);
int ctn_conv1x1_backward(const ctn_rows_desc* d, int cout, const void* x, const float* w, const void* gy, void* gx,
                         float* gw, void* ws, size_t ws_bytes, void* stream);

/* mask nonlinearity (conv_tasnet.py:202-208) over nspk speakers of score rows
 * [M*Kp][nspk*N] (d->C = nspk*N, channel s*N + n as score.view(M, C, N, K)) */
int ctn_mask_forward(const ctn_rows_desc* d, int nspk, int mask_type, const void* score, void* mask, void* stream);
int ctn_mask_backward(const ctn_rows_desc* d, int nspk, int mask_type, const void* score, const void* gmask,
                      void* gscore, void* stream);

/* -------------------------------------------------------------------------
 * Streaming causal separation: replaces running src/separate.py:35-79 on a
 * causal model (conv_tasnet.py:176 Chomp1d, :289) whole-signal, with chunked
 * calls that carry state instead of re-running history.  fp32.
 * Frame k of a stream covers samples [k*L/2, k*L/2 + L).  State per
 * TemporalBlock: `ring` [M][ring_frames][H], the block's depthwise-conv input
 * frames (after conv1x1, PReLU and norm 1), frame g at slot g % ring_frames;
 * ring_frames a power of two >= (P-1)*dilation + K.  `pos` = frames of this
 * stream processed before the call (taps before frame 0 read as zero: the
 * reference's causal zero padding).  1x1 weights are passed TRANSPOSED,
 * [in][out]: wb_t [N][B], w1_t [B][H], w2_t [H][B], wm_t [B][C*N]; wd [H][P];
 * U [N][L]; V [L][N] (Linear(N, L).weight).  norm CTN_NORM_CLN takes
 * gamma/beta, CTN_NORM_BN an eval-mode BatchNorm folded to scale/shift.
 * encode: samples [M][ld] (the call's (K-1)*L/2 + L samples at offset 0)
 *         -> w_out [M][K][N] (ReLU(U*frame)), x_out [M][K][B] (cLN, bottleneck)
 * block : x_in [M][K][B] -> ring (new frames), x_out [M][K][B]
 * decode: x_last, w -> out [M][C][K*L/2]: the K frames overlap-added with
 *         tail_in [M][C][L/2] (zeros at the stream start); tail_out gets the
 *         last frame's second half.  frames_ws: [M][C][K][L] scratch.
 * ------------------------------------------------------------------------- */
typedef struct {
  int32_t M, K;
  int32_t N, L, B, H, P, C;
  int32_t norm;      /* CTN_NORM_CLN or CTN_NORM_BN (eval, affine) */
  int32_t mask_type; /* ctn_mask_type or CTN_MASK_IDENTITY */
} ctn_stream_desc;
int ctn_stream_encode(const ctn_stream_desc* d, const float* samples, int64_t ld_samples, const float* U,
                      const float* gamma0, const float* beta0, const float* wb_t, float* w_out, float* x_out,
                      void* stream);
int ctn_stream_block(const ctn_stream_desc* d, int dilation, int64_t pos, int ring_frames, const float* x_in,
                     const float* w1_t, const float* alpha1, const float* norm1_a, const float* norm1_b,
                     const float* wd, const float* alpha2, const float* norm2_a, const float* norm2_b,
                     const float* w2_t, float* ring, float* x_out, void* stream);
int ctn_stream_decode(const ctn_stream_desc* d, const float* x_last, const float* w, const float* wm_t,
                      const float* V, const float* tail_in, float* tail_out, float* frames_ws, float* out,
                      void* stream);

/* ABI v7: one whole call (encode, every TemporalBlock, decode) in one entry, its 1x1
 * convs split over 32-output column chunks so that a call with few new frames spreads
 * over many CUs (the v5 entries give each (stream, 8 frames) one workgroup that streams
 * every 1x1 weight through one CU).  Same state and layouts as the v5 entries; `blocks`
 * is a HOST array of nblocks per-block parameter sets (separator order), each with its
 * own ring.  `pos` as above; `tail_in` / `tail_out` [M][C][L/2] must not alias.
 * `ws` >= ctn_stream_workspace_bytes(d).  Same arithmetic as the v5 path (the 1x1 sums
 * are added in another order: results agree to fp32 rounding). */
typedef struct {
  int32_t dilation, ring_frames;
  const float* w1_t;     /* [B][H] */
  const float* alpha1;
  const float* norm1_a;
  const float* norm1_b;
  const float* wd;       /* [H][P] */
  const float* alpha2;
  const float* norm2_a;
  const float* norm2_b;
  const float* w2_t;     /* [H][B] */
  float* ring;           /* [M][ring_frames][H] */
} ctn_stream_block_params;
typedef struct {
  const float* U;        /* [N][L] */
  const float* gamma0;   /* separator cLN */
  const float* beta0;
  const float* wb_t;     /* [N][B] */
  const float* wm_t;     /* [B][C*N] */
  const float* V;        /* [L][N] */
  const ctn_stream_block_params* blocks;
  int32_t nblocks;
} ctn_stream_model;
size_t ctn_stream_workspace_bytes(const ctn_stream_desc* d);
int ctn_stream_call(const ctn_stream_desc* d, const ctn_stream_model* model, int64_t pos, const float* samples,
                    int64_t ld_samples, const float* tail_in, float* tail_out, float* out, void* ws,
                    size_t ws_bytes, void* stream);

/* Kernel plan of one TemporalBlock launch (no device work): writes a NUL-terminated list
 * "step=kernel,..." of the kernels ctn_tblock_forward (backward = 0) or the backward entries
 * (backward = 1) would choose for d, e.g. "pairA=dual_ws,dw_bwd=wave,gx=ws_n1bwd,dW1=cols".
 * Shapes outside a kernel's limits (tensors of 2^31 bytes or more for the persistent
 * kernels' 32-bit offsets) fall back to the tiled kernels; this is how a caller sees it. */
int ctn_tblock_plan(const ctn_tblock_desc* d, int backward, char* out, size_t cap);

/* -------------------------------------------------------------------------
 * Opt-in kernel timer (bench.py roofline; the reference has no counterpart — its
 * solver prints epoch wall time only, src/solver.py:178-188): when enabled, every
 * launch of a selected kernel family is bracketed by hipEvents on its stream.
 * Kinds of the TemporalBlock (conv_tasnet.py:212-272):
 * ------------------------------------------------------------------------- */
enum {
  CTN_TIMER_GEMM1 = 1,     /* forward first 1x1 (B -> H, PReLU-statistics epilogue)       */
  CTN_TIMER_DW_FWD = 2,    /* depthwise forward (norm 1 applied, PReLU-2 statistics)      */
  CTN_TIMER_GEMM_A = 3,    /* backward pair A: g_n2 = gy.W2 (+ dW2 on the dual kernel)     */
  CTN_TIMER_DW_BWD = 4,    /* depthwise backward (norm-2 / PReLU-2 backward, dW_dw, sums)  */
  CTN_TIMER_GEMM_GX = 5,   /* backward gx = n1bwd(g).W1 + gy (stores dL/dh1)              */
  CTN_TIMER_COLS_W1 = 6,   /* backward dW1 = (dL/dh1)^T . x column GEMM                   */
  CTN_TIMER_GEMM2 = 7      /* forward second 1x1 (H -> B, norm 2 applied, residual)       */
};
/* one kind (0 = off), or a set of kinds (bit k = kind k; max_launches per kind) */
int ctn_timer_enable(int kind, int max_launches);
int ctn_timer_enable_mask(uint32_t mask, int max_launches);
int ctn_timer_read(double* total_ms, int* launches);              /* all kinds */
int ctn_timer_read_kind(int kind, double* total_ms, int* launches);
/* ABI v11: bracket only every stride-th launch of each enabled kind (stride >= 1,
 * default 1; counted from the last enable).  Each bracketing event pair leaves the GPU
 * idle for a few microseconds around the launch, so a sampled timer perturbs the
 * measured run less; read_kind then reports the sampled launches. */
int ctn_timer_set_stride(int stride);
/* ABI v11: a streaming device-to-device copy (16 B per lane, `workgroups` x 256 threads,
 * grid-stride), bench.py's measured bandwidth ceiling beside the datasheet peak.  bytes,
 * dst and src must be multiples of 16.  flags: bit 0 nontemporal loads and stores, bit 1
 * eight loads in flight per lane instead of four. */
#define CTN_COPY_NT 1
#define CTN_COPY_DEEP 2
int ctn_copy_bytes(void* dst, const void* src, size_t bytes, int workgroups, int flags, void* stream);
/* ABI v12: an MFMA throughput microbenchmark (bench.py's measured matrix peak beside the
 * 2.5 PF/s datasheet value): `workgroups` x 4 waves, each issuing `iters` rounds of
 * independent back-to-back bf16 MFMAs on random register operands — shape 0
 * v_mfma_f32_16x16x32_bf16 (8 accumulators), 1 v_mfma_f32_32x32x16_bf16 (4) — writing
 * workgroups*256 floats to `out`; *flops (may be NULL) = the FLOP of the launch. */
int ctn_mfma_peak(int shape, int workgroups, int iters, float* out, double* flops, void* stream);

/* -------------------------------------------------------------------------
 * Device error word (ABI v9).  Kernels whose waves hand tiles to each other through
 * LDS generation words (the wave-specialised dual GEMM of ctn_tblock_backward*, the
 * ring variant of the weight-stationary GEMM) bound every wait; a wait that runs out
 * sets bit CTN_DEVERR_SPIN and the launch's outputs are invalid.  The word is copied
 * to the host asynchronously at the end of every ctn_tblock_reduce_grads, which fails
 * with CTN_ERR_HIP at its next call once a bit is set.  ctn_device_status
 * synchronises `stream`, returns the word in *word (may be NULL) and CTN_ERR_HIP when
 * it is non-zero; clear != 0 resets it.
 * ------------------------------------------------------------------------- */
#define CTN_DEVERR_SPIN 1u
int ctn_device_status(void* stream, uint32_t* word, int clear);

#ifdef __cplusplus
}
#endif
#endif /* CTN_H */
