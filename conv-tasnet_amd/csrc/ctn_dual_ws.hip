// Dual GEMM, bf16, gfx950: a row GEMM and the weight gradient that shares its A stream,
// in one pass over the frame rows.  It runs the TemporalBlock backward's second 1x1 conv
// ("pair A", conv_tasnet.py:256-263 backward) in one pass over gy and d:
//   C        = g_n2 = gy . W2                    (dL/d norm-2 output, stored bf16)
//   grp_slab : norm-2 backward sums of (g_n2*gamma2, g_n2*gamma2*hat a2)
//   Dpart    = gy^T . (gamma2 * hat a2 + beta2)  (dW2 partial per row range)
// with hat a2 = (PReLU(d) - mean) * rstd (gLN per utterance or cLN per frame row).
// Without the fusion these are two kernels (row GEMM + column GEMM), and gy and d stream
// from HBM twice.
//
// Operands (GemmDual, ctn_kernels.h; every matrix bf16, row-major, rows = M * Kp frame rows):
//   A  = gy  [rows][lda], Kred = 256 channels; rows of padded frames (k >= K) read as zeros
//   W  = W2^T [Nout][ldw]; Wf, when given, the same weight in MFMA fragment order
//        (frag_offset: 1 KiB contiguous per wave and fragment)
//   Bm = d   [rows][ldb], the raw pre-activation: the PReLU + norm + affine of the column
//        operand and the PReLU + norm of the epilogue's hat a2 are both applied to it in
//        registers (R is not read)
//   stats = bop.stats: (mean, rstd) float2 per utterance [M] (gLN) or per frame row [rows]
//        (cLN; padded frames' entries are not finite and are masked); gamma, bop.gamma,
//        bop.beta [Nout] and alpha, bop.alpha [1] fp32
// Outputs:
//   C     [rows][ldc] bf16
//   Dpart [range][Kred][Nout] fp32: one partial per row range, stored once per workgroup
//         and summed over the ranges by slab_reduce in a fixed order
//   grp_slab double2 (sum, sum of squares):
//         gLN: [((range * S + slice) * DV_NR + row wave)][kmax], one entry per utterance
//              run of the wave's tiles (the WsRuns layout of ctn_common.h, waves = S * DV_NR);
//         cLN: [row][S], the four row waves' partials combined in LDS in the order 0..3.
// Nothing is accumulated with atomics: every partial has one writer and every consumer
// (slab_reduce, StatFold, stats_finalize) adds them in a fixed order, so all outputs are
// bitwise reproducible.
//
// Decomposition.  The output channels are cut into S = Nout / 128 slices.  Workgroup
// (row range, slice) keeps its slice of W resident in VGPRs (MFMA A-fragments, as the
// weight-stationary kernel ctn_gemm_ws.hip) and its Dpart slice [256][128] as fp32 MFMA
// accumulators, and streams the 32-row tiles of its range (the ranges split the tiles
// evenly; 256 / S of them, or one per tile when there are fewer tiles).  Hardware
// workgroup ids are dealt round-robin over the 8 XCDs, so when the grid is a multiple of
// 8 S the S workgroups of one row range are given ids 8 apart and sit on the same XCD:
// each gy tile is fetched from HBM once and re-read by the other slices from that XCD's L2.
// Per tile the row part is v_mfma_f32_16x16x32_bf16 against the resident W slice with the
// epilogue straight from the accumulators, and the column part is
// Dpart += gy_tile^T . op(d)_tile with both operands read by ds_read_b64_tr_b16 (the
// reduction runs over the tile's frame rows).
//
// Schedule.  A kernel that takes every wave through one barrier per tile (wait for the
// tile's LDS-DMA, then staging, MFMA and epilogue in lockstep) makes the phases add up
// (DESIGN.md §10-11).  Here the roles are split inside the workgroup (16 waves, 4 per SIMD):
//   * 4 memory waves LDS-DMA the tiles PF tiles ahead into an LDS ring of NSL slots
//     (A = gy in MFMA fragment order, B = raw d of the slice, the tile's statistics),
//     wait for their own DMA with a counted vmcnt and publish FULL;
//   * 4 row waves (32 output channels each, resident W2 fragments) run the row GEMM of
//     both 16-row blocks and the norm-2 backward epilogue (hat a from raw d in fp32),
//     store C straight to memory and publish DONE;
//   * 8 column waves accumulate the dW2 slice (64 x 64 each) as MFMA accumulators from
//     A and op(d) (PReLU + norm + affine, bf16, applied to their B fragments) and publish
//     DONE.
// FULL / DONE are one generation word per wave per slot in LDS (a memory wave waits
// for every DONE of tile t-NSL before refilling its slot), so the MFMAs of one tile
// overlap the DMA and transforms of the next ones, and no wave ever waits on another
// wave's memory operations.  Every LDS read of another wave's data happens after that
// wave's `s_waitcnt lgkmcnt(0)` + generation-word store and this wave's matching
// generation-word load.
#include <stdlib.h>

#include "ctn_common.h"
#include "ctn_kernels.h"

namespace ctn {

namespace {

constexpr int DV_TM = 32;                        // frame rows per tile
// 8 column waves (64 dW2 accumulators each, 4 waves per SIMD, 128 VGPRs per wave): 84 us
// against 86-91 with 4 waves of 128 accumulators
constexpr int DV_NR = 4, DV_NC = 8, DV_NMW = 4;  // row / column / memory waves
constexpr int DV_ND = DV_NR + DV_NC;             // waves that publish DONE
// The statistics partials follow from the row waves: gLN one run list per (range, slice,
// row wave), cLN one entry per (row, slice) (the row waves' partials are combined in LDS).
// Round 6 measured two other gLN forms, both bit-identical and slower, and removed them
// (DESIGN.md §16): eight row waves with the tile DMA in the column waves (commit 9656623)
// and the row epilogue in the memory waves (commit 9d56d29).
constexpr int DV_CLN_PARTS = 1;                  // cLN statistics entries per (row, slice)
constexpr int DV_NT = (DV_ND + DV_NMW) * 64;     // 1024 threads
constexpr int DV_KB = 8, DV_KR = 256;            // reduction of the row part (gy channels)
constexpr int DV_NS = 128;                       // output channels per slice
constexpr int DV_GRID = 256;
// Slot layout: the B image holds the raw d slice exactly as the LDS-DMA lands it
// (row-major, 16-byte granules swizzled per row); the column waves apply PReLU + norm +
// affine to their B fragments, the row waves read raw d from it, a slot is 24.8 KB and the
// ring holds 6 tiles.  79.5 us against 99.5 with op(d) written by the memory waves into
// 33 KB slots, ring of 4.
constexpr int DV_NSL = 6;                        // LDS ring slots
// tiles a memory wave keeps in flight ahead of the one being consumed (<= NSL - 1: the
// slot refilled is the one the consumers released last); gLN and cLN forms alike
constexpr int DV_PF = DV_NSL - 1;
static_assert(DV_PF >= 1 && DV_PF <= DV_NSL - 1, "ring look-ahead");
// Column-wave split of the 256 x 128 dW2 slice: each of the 8 waves owns CJ 16-column
// blocks x (16 / CJ) 16-row blocks (64 accumulator registers either way).  Fewer column
// blocks per wave means fewer waves share and transform each B fragment, at the price of
// more A fragment reads per wave: CJ=1 79.5 us, CJ=2 85.0 (bench shape).
constexpr int DV_CJ = 1;

// Static wave priority per role (s_setprio once at the role's start).  The SIMD's issue
// arbiter serves the higher priority first, so the memory wave sharing a SIMD with three
// consumers issues each tile's LDS-DMA as soon as its slot is free instead of behind the
// consumers' MFMA/VALU streams, and the row waves (whose stores feed the next kernel) go
// before the column waves.  Measured (microbenchmark, bench shape, three alternations on
// one box): gLN 81-89 us with none, 75-78 us with memory 3 + row 1; higher
// column priority slower (89-92 us); the c5 shape 84 -> 76 us; the cLN form (c4) flat to
// slightly slower, so it keeps none.
constexpr int DV_PRIO_ROW = 1, DV_PRIO_MEM = 3;   // gLN only
template <int PR, int NK> CTN_DEV void dv_prio() {
  if constexpr (NK == NORM_GLN) __builtin_amdgcn_s_setprio(PR);
}

// Row waves: A fragments read LA k-steps ahead of their MFMAs
constexpr int DV_LA = 1;

// Bound-finding builds only (tools/microbench/dual_ws_bench.hip -DCTN_DV_EXP=<bits>):
// bit 0 consumers skip all arithmetic (wait FULL, publish DONE), bit 1 no column part,
// bit 2 no epilogue math, bit 3 no C stores, bit 4 row waves store zeros and nothing else,
// bit 5 the memory waves issue no DMA (consumers read whatever the ring holds), bit 6 the
// row waves skip all arithmetic.
#ifndef CTN_DV_EXP
#define CTN_DV_EXP 0
#endif

// Diagnostic build only (tools/microbench/dual_ws_bench.hip -DCTN_DV_STAMP=1): per wave,
// s_memtime cycles spent in each wait (row/column: FULL polls; memory: own-DMA vmcnt
// waits and DONE polls) and in the whole tile loop, summed into dv_stamps[wg][wave][4]
#ifndef CTN_DV_STAMP
#define CTN_DV_STAMP 0
#endif
#if CTN_DV_STAMP
__device__ unsigned long long dv_stamps[1024 * 16 * 4];
#define DV_TS(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define DV_ACC(i, t0v) st_acc[i] += __builtin_amdgcn_s_memtime() - (t0v)
#define DV_STAMP_DECL unsigned long long st_acc[4] = {0, 0, 0, 0}
#define DV_STAMP_STORE                                                                    \
  do {                                                                                    \
    if (lane == 0)                                                                        \
      for (int i_ = 0; i_ < 4; ++i_) dv_stamps[((size_t)blockIdx.x * 16 + wid) * 4 + i_] = st_acc[i_]; \
  } while (0)
#else
#define DV_TS(v) \
  do {           \
  } while (0)
#define DV_ACC(i, t0v) \
  do {                 \
  } while (0)
#define DV_STAMP_DECL \
  do {                \
  } while (0)
#define DV_STAMP_STORE \
  do {                 \
  } while (0)
#endif

// slot layout (bytes)
constexpr int DV_A = DV_TM * DV_KR * 2;          // 16384: gy tile, MFMA fragment-order image
constexpr int DV_B = DV_TM * DV_NS * 2;          // raw d slice, 256-byte rows (dv_rbgr)
constexpr int DV_ST = 256;                       // statistics
constexpr int OFF_A = 0, OFF_B = OFF_A + DV_A, OFF_ST = OFF_B + DV_B;
constexpr int DV_SLOT = OFF_ST + DV_ST;

// B image: granule g of row r at r * 256 + 16 * position, position = g's low bit
// and (g/2) XOR a 3-bit row hash.  The hash differs between the 8 rows a column wave's
// transposed 8-byte reads touch in one half-wave ({q, 8+q} or {4+q, 12+q}, q < 4, and the
// same + 16), so those 32 reads hit 32 distinct 8-byte bank pairs; a row wave's 16-byte
// reads of 16 rows see at most 2-way conflicts.
CTN_DEV int dv_rbhash(int r) { return (r & 3) | (((r >> 3) & 1) << 2); }
CTN_DEV int dv_rbpos(int r, int g) { return (g & 1) | ((((g >> 1) ^ dv_rbhash(r)) & 7) << 1); }
CTN_DEV int dv_rbgr(int r, int g) { return r * 256 + (dv_rbpos(r, g) << 4); }
// counted wait with a compile-time count (the steady state of the ring: a runtime switch
// over the count compiles to ~300 scalar instructions per tile)
template <int N> CTN_DEV void dv_vmwait_c() {
  static_assert(N >= 0 && N < 64, "vmcnt range");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <bool LE1> CTN_DEV float dv_prelu(float x, float al) { return prelu_nq<LE1>(x, al); }

CTN_DEV s16x4_t dv_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(p));
}

// Generation words.  Every lane reads the same word (wave-uniform by readfirstlane);
// the poll is followed by a compiler barrier so no LDS read of the published data is
// issued before the word that publishes it has been seen (LDS executes one wave's
// DS instructions in order).
// The spin is bounded (CTN_SPIN_LIMIT polls, about 0.2 s): a protocol error sets
// CTN_DEVERR_SPIN in the device error word (p.err, ctn_device_status) and the launch
// ends, reported as failed by the host, instead of a wave that never finishes.
// (Volatile accesses keep their address space only through an explicitly LDS-typed
// pointer: through a generic one they become FLAT operations, whose waits drain every
// outstanding global load of the wave.)
typedef __attribute__((address_space(3))) volatile v4u lds_v4u;
typedef __attribute__((address_space(3))) volatile uint32_t lds_u32;
template <int N> CTN_DEV void dv_wait(const uint32_t* f, uint32_t gen, uint32_t* err) {
  static_assert(N % 4 == 0, "generation words per slot: whole 16-byte reads");
  const lds_v4u* fl = (const lds_v4u*)(f);
  uint32_t it = 0;
  for (; it < CTN_SPIN_LIMIT; ++it) {
    uint32_t mn = 0xffffffffu;
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const v4u a = fl[i];
      mn = min(mn, min(min(a[0], a[1]), min(a[2], a[3])));
    }
    if (__builtin_amdgcn_readfirstlane(mn) >= gen) break;
    __builtin_amdgcn_s_sleep(1);
  }
  if (it == CTN_SPIN_LIMIT) spin_timeout(err);
  asm volatile("" ::: "memory");
}
// publish: this wave's LDS writes (and reads) complete, then the generation word
CTN_DEV void dv_signal(uint32_t* f, uint32_t gen) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  *(lds_u32*)(f) = gen;
  asm volatile("" ::: "memory");
}

// 16 waves: row waves 0-3, column waves 4-11, memory waves 12-15
template <int NK, int NSL, int PF>
__global__ __launch_bounds__(DV_NT) void gemm_dual_ws_kernel(GemmDual p) {
  constexpr int NR = DV_NR, ND = DV_ND;
  constexpr int TM = DV_TM, KB = DV_KB, KR = DV_KR, NS = DV_NS;
  constexpr int SLOT = DV_SLOT;
  static_assert(NSL * SLOT <= 160 * 1024 - 2048, "LDS budget");
  __shared__ __attribute__((aligned(16))) char smem[NSL * SLOT];
  __shared__ __attribute__((aligned(16))) uint32_t fl_full[NSL][4];   // per memory wave
  __shared__ __attribute__((aligned(16))) uint32_t fl_done[NSL][ND];   // per row / column wave
  __shared__ __attribute__((aligned(16))) float sgb[2][NS];            // gamma2 / beta2 of the slice
  // cLN: the four row waves' per-row partials of a tile, combined in LDS before storing
  // (S entries per row instead of 4 S), two tiles deep, and one generation
  // word per (buffer, row wave)
  constexpr bool CLNC = NK == NORM_CLN;
  __shared__ __attribute__((aligned(16))) double2 cln_scr[CLNC ? 2 : 1][CLNC ? DV_NR * DV_TM : 1];
  __shared__ __attribute__((aligned(16))) uint32_t fl_rows[2][4];

  // wave id through readfirstlane: wave-uniform to the compiler, so per-role pointers and
  // offsets live in SGPRs (the row waves are at the 128-VGPR limit of 4 waves per SIMD)
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int S = p.Nout / NS;
  const int nr = (int)gridDim.x / S;   // row ranges
  int rr, sl;
  {
    const int b = (int)blockIdx.x;
    if ((int)gridDim.x % (8 * S) == 0) {   // the S slices of a range on one XCD (L2 shares gy)
      const int l = b / 8;
      sl = l % S;
      rr = (b % 8) * (nr / 8) + l / S;
    } else {
      sl = b % S;
      rr = b / S;
    }
  }
  const long rows = p.g.rows();
  const int ntile = (int)(rows / TM);
  const int t0 = (int)((long)ntile * rr / nr), t1 = (int)((long)ntile * (rr + 1) / nr);
  const int n0 = sl * NS;
  const int Kp = p.g.Kp, Kv = p.g.K, tpu = Kp / TM;

  if (tid < NSL * 4) (&fl_full[0][0])[tid] = 0u;
  else if (tid < NSL * (4 + ND)) (&fl_done[0][0])[tid - NSL * 4] = 0u;
  else if (tid < NSL * (4 + ND) + 8) (&fl_rows[0][0])[tid - NSL * (4 + ND)] = 0u;
  if (tid < 2 * NS) sgb[tid / NS][tid % NS] = (tid < NS ? p.bop.gamma : p.bop.beta)[n0 + tid % NS];
  __syncthreads();

  const float eal = p.alpha[0];
  const int kmax = ws_runs_kmax(ntile, nr, tpu);
  if (wid < NR) {
    // ======================= row waves =======================
    dv_prio<DV_PRIO_ROW, NK>();
    // wave r: output channels n0 + 32r .. +31 of both 16-row blocks of every tile, against
    // the resident W fragments (group 4*sl + r of the fragment-ordered copy, nb = 0, 1):
    // lane (lg, lr) holds channels 32r + 8lg .. +7 (slice-local) of frame rows lr, 16 + lr.
    const int r = wid;
    v4u wf[2][KB];
    const bf16raw* WF = reinterpret_cast<const bf16raw*>(p.Wf);
    const bf16raw* W = reinterpret_cast<const bf16raw*>(p.W);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int n = n0 + 32 * r + (lr >> 2) * 8 + nb * 4 + (lr & 3);
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        wf[nb][kb] = WF ? ldg16(WF + frag_offset(4 * sl + r, nb, kb, lane, KR))
                        : ldg16(W + (size_t)n * p.ldw + kb * 32 + lg * 8);
    }
    const int cl = 32 * r + 8 * lg;
    bf16raw* Cg = reinterpret_cast<bf16raw*>(p.C);
    // gamma2 of the lane's 8 channels
    float gam[8];
    *reinterpret_cast<float4*>(gam) = *reinterpret_cast<const float4*>(p.gamma + n0 + cl);
    *reinterpret_cast<float4*>(gam + 4) = *reinterpret_cast<const float4*>(p.gamma + n0 + cl + 4);
    const int rbase = lg * 256 + ((lr ^ ((lg & 1) * 12)) << 4);   // + rb * KB * 1024 + kb * 1024
    const int ro = OFF_B + dv_rbgr(lr, 4 * r + lg);                // row lr; row 16 + lr at + 4096

    DV_STAMP_DECL;
    double run_s = 0.0, run_q = 0.0;
    const int m0 = t0 / tpu;
    int run_m = m0;
    double2* run_slab = p.grp_slab + (((size_t)rr * S + sl) * DV_NR + r) * kmax;
    auto flush = [&]() __attribute__((always_inline)) {
      const double s = wave_sum_dpp_d(run_s), ss = wave_sum_dpp_d(run_q);
      run_slab[run_m - m0] = make_double2(s, ss);
    };
    auto run = [&](auto le1) __attribute__((always_inline)) {
      constexpr bool LE1 = decltype(le1)::value;
      int slot = 0;
      uint32_t gen = 1;
      DV_TS(tl0);
      for (int t = t0; t < t1; ++t) {
        DV_TS(tw0);
        dv_wait<4>(fl_full[slot], gen, p.err);
        DV_ACC(0, tw0);
        char* base = smem + slot * SLOT;
        if constexpr (CTN_DV_EXP & 16) {   // C stores only (zeros)
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) stg16(Cg + ((size_t)t * TM + 16 * rb + lr) * p.ldc + n0 + cl, v4u{0u, 0u, 0u, 0u});
        } else if constexpr (!(CTN_DV_EXP & 65)) {
          f32x4_t acc[2][2];
#pragma unroll
          for (int rb = 0; rb < 2; ++rb)
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[rb][nb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          // the A fragments of k-step kb + LA are read while the MFMAs of kb run (the
          // interleave pinned below: the register-pressure scheduler would otherwise pull
          // each read down to its MFMAs and expose every read's latency)
          constexpr int LA = DV_LA;
          v4u bw[LA + 1][2];
          auto rd = [&](int kb) __attribute__((always_inline)) {
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
              bw[kb % (LA + 1)][rb] = *reinterpret_cast<const v4u*>(base + OFF_A + rb * KB * 1024 + rbase + kb * 1024);
          };
#pragma unroll
          for (int kb = 0; kb < LA && kb < KB; ++kb) rd(kb);
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) {
            if (kb + LA < KB) rd(kb + LA);
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
              const v4u b = bw[kb % (LA + 1)][rb];
#pragma unroll
              for (int nb = 0; nb < 2; ++nb)
                acc[rb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wf[nb][kb]),
                                                                      __builtin_bit_cast(bf16x8_t, b), acc[rb][nb], 0, 0, 0);
            }
          }
          if constexpr (LA > 0) {
            __builtin_amdgcn_sched_group_barrier(0x100, 2 * (LA < KB ? LA : KB), 0);
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
              if (kb + LA < KB) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
              __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
          }
          // ---- epilogue: norm-2 backward sums, C image (16 bytes per lane and row).
          // (Summing ga * a and scaling by rstd once per row saves one FMA per element but
          // cancels when |mean| >> the spread of a: not used.)
          float s1[2] = {0.f, 0.f}, q1[2] = {0.f, 0.f};
#pragma unroll
          for (int rb = 0; rb < 2; ++rb) {
            const v4u rw = *reinterpret_cast<const v4u*>(base + ro + rb * 4096);
            float2 est;
            if constexpr (NK == NORM_GLN) est = *reinterpret_cast<const float2*>(base + OFF_ST);   // the tile's utterance
            else est = *reinterpret_cast<const float2*>(base + OFF_ST + (16 * rb + lr) * 8);
            const float rs = est.y, ms = -est.x * est.y;
            const bool ok = NK == NORM_GLN || (t * TM) % Kp + 16 * rb + lr < Kv;   // cLN padded frames: stats not finite
            float f[8];
            unpack_bf16x8(rw, f);
            if constexpr (!(CTN_DV_EXP & 4)) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float a = dv_prelu<LE1>(f[e], eal);
                const float ah = ok ? fmaf(a, rs, ms) : 0.f;   // hat a
                const float ga = acc[rb][e >> 2][e & 3] * gam[e];
                s1[rb] += ga;
                q1[rb] = fmaf(ga, ah, q1[rb]);
              }
            }
            const v4u cv = {pk_bf16(acc[rb][0][0], acc[rb][0][1]), pk_bf16(acc[rb][0][2], acc[rb][0][3]),
                            pk_bf16(acc[rb][1][0], acc[rb][1][1]), pk_bf16(acc[rb][1][2], acc[rb][1][3])};
            // whole 16-byte lanes straight to memory (a wave covers 16 rows x 64 B)
            if constexpr (!(CTN_DV_EXP & 8))
              // wave-uniform 64-bit tile base + 32-bit lane offset (SGPR base, one VGPR)
              stg16(Cg + (size_t)t * TM * p.ldc + n0 + (uint32_t)((16 * rb + lr) * p.ldc + cl), cv);
          }
          if constexpr (NK == NORM_GLN) {
            const int m = t / tpu;
            if (m != run_m) {
              flush();
              run_s = run_q = 0.0;
              run_m = m;
            }
            run_s += (double)(s1[0] + s1[1]);
            run_q += (double)(q1[0] + q1[1]);
          } else {
            // per-row partial over this wave's 32 channels into LDS; once all four row
            // waves have written theirs, wave r sums rows 8r .. 8r+7 over the waves in
            // order 0..3 and stores one entry per (row, slice): a quarter of the
            // statistics bytes the finalize reads
            const int k = t - t0, bsel = k & 1;
            const uint32_t rgen = (uint32_t)(k >> 1) + 1u;
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
              const float s = xsum_rows(s1[rb]), ss = xsum_rows(q1[rb]);
              if (lg == 0) cln_scr[bsel][r * TM + 16 * rb + lr] = make_double2((double)s, (double)ss);
            }
            dv_signal(&fl_rows[bsel][r], rgen);
            dv_wait<4>(fl_rows[bsel], rgen, p.err);
            if (lane < 8) {
              const int row = 8 * r + lane;
              double s = 0.0, ss = 0.0;
#pragma unroll
              for (int w = 0; w < DV_NR; ++w) {
                const double2 v = cln_scr[bsel][w * TM + row];
                s += v.x;
                ss += v.y;
              }
              p.grp_slab[((size_t)t * TM + row) * S + sl] = make_double2(s, ss);
            }
          }
        }
        dv_signal(&fl_done[slot][r], gen);
        if (++slot == NSL) {
          slot = 0;
          ++gen;
        }
      }
      DV_ACC(3, tl0);
    };
    if (t0 < t1) {
      if (eal <= 1.f) run(std::true_type{});
      else run(std::false_type{});
      if constexpr (NK == NORM_GLN) flush();
    }
    DV_STAMP_STORE;
    return;
  }
  if (wid < ND) {
    // ======================= column waves =======================
    // wave c = (wp, wn) owns dW2 blocks p in [16 CI wp, +16 CI), n in [n0 + 16 CJ wn, +16 CJ):
    // dW2 += gy_tile^T . op(d)_tile, the reduction over the tile's 32 frame rows
    // the slice's 16 x 8 blocks of 16 x 16: waves in a (NC / (8 / CJ)) x (8 / CJ) grid,
    // each CI x CJ blocks
    constexpr int CJ = DV_CJ, CI = 16 * (8 / CJ) / DV_NC;
    static_assert(CI >= 2 && CI <= 16 && CI % 2 == 0, "column split");
    const int c = wid - NR, wp = c / (8 / CJ), wn = c % (8 / CJ);
    DV_STAMP_DECL;
    f32x4_t dacc[CI][CJ];
#pragma unroll
    for (int i = 0; i < CI; ++i)
#pragma unroll
      for (int j = 0; j < CJ; ++j) dacc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // lane-constant LDS addresses (A: the fragment-order image, 16-row block mb and k-block
    // kb of 1 KiB, 16-byte chunk lg at 256 lg, frame row r at 16 (r ^ (lg odd ? 12 : 0));
    // B: row-major granules, block j at bbase ^ (j << 5))
    const int q = lr >> 2, pp = lr & 3;
    int abase[2], bbase[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = 8 * lg + 4 * h + q;
      abase[h] = (lg >> 1) * KB * 1024 + (CI / 2) * wp * 1024 + (pp >> 1) * 256 + (((row & 15) ^ ((pp >> 1) * 12)) << 4) +
                 (pp & 1) * 8;
      bbase[h] = dv_rbgr(row, 2 * CJ * wn + (pp >> 1)) + 8 * (pp & 1);
    }
    // the B fragment of block j holds raw d of column 16 (CJ wn + j) + lr (slice-local)
    // at frame rows 8 lg .. 8 lg + 7; op(d) is applied here, per element in fp32:
    // fma(PReLU(d) - mean, rstd * gamma2, beta2), rounded to bf16 (to nearest even); zero
    // on cLN's padded frames
    float cg[CJ], cb[CJ];
#pragma unroll
    for (int j = 0; j < CJ; ++j) {
      cg[j] = sgb[0][16 * (CJ * wn + j) + lr];
      cb[j] = sgb[1][16 * (CJ * wn + j) + lr];
    }
    const float bal = p.bop.alpha[0];
    // one tile's B fragments (raw d -> op(d)), read from the ring slot at `base`
    auto load_b = [&](auto le1, int t, const char* base, bf16x8_t* bfr) __attribute__((always_inline)) {
      constexpr bool LE1 = decltype(le1)::value;
      const char* bb = base + OFF_B;
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        const s16x4_t lo = dv_tr(bb + (bbase[0] ^ (j << 5)));
        const s16x4_t hi = dv_tr(bb + (bbase[1] ^ (j << 5)));
        bfr[j] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
      float mu[8], rs[8];
      if constexpr (NK == NORM_GLN) {
        const float2 st = *reinterpret_cast<const float2*>(base + OFF_ST);
#pragma unroll
        for (int e = 0; e < 8; ++e) mu[e] = st.x, rs[e] = st.y;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float4 st = *reinterpret_cast<const float4*>(base + OFF_ST + 64 * lg + 16 * k);
          mu[2 * k] = st.x, rs[2 * k] = st.y, mu[2 * k + 1] = st.z, rs[2 * k + 1] = st.w;
        }
      }
      const int tk = (t * TM) % Kp;
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        v4u v = __builtin_bit_cast(v4u, bfr[j]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float x0 = __uint_as_float(v[k] << 16), x1 = __uint_as_float(v[k] & 0xffff0000u);
          x0 = dv_prelu<LE1>(x0, bal);
          x1 = dv_prelu<LE1>(x1, bal);
          x0 = fmaf(x0 - mu[2 * k], rs[2 * k] * cg[j], cb[j]);
          x1 = fmaf(x1 - mu[2 * k + 1], rs[2 * k + 1] * cg[j], cb[j]);
          if constexpr (NK == NORM_CLN) {   // padded frames: statistics not finite
            if (tk + 8 * lg + 2 * k >= Kv) x0 = 0.f;
            if (tk + 8 * lg + 2 * k + 1 >= Kv) x1 = 0.f;
          }
          v[k] = pk_bf16(x0, x1);
        }
        bfr[j] = __builtin_bit_cast(bf16x8_t, v);
      }
    };
    auto a_frag = [&](const char* base, int i) __attribute__((always_inline)) {
      const int o = (i >> 1) * 1024 + (i & 1) * 512;
      const s16x4_t lo = dv_tr(base + OFF_A + abase[0] + o), hi = dv_tr(base + OFF_A + abase[1] + o);
      return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    auto run = [&](auto le1) __attribute__((always_inline)) {
      int slot = 0;
      uint32_t gen = 1;
      DV_TS(tl0);
      for (int t = t0; t < t1; ++t) {
        DV_TS(tw0);
        dv_wait<4>(fl_full[slot], gen, p.err);
        DV_ACC(0, tw0);
        const char* base = smem + slot * SLOT;
        if constexpr (!(CTN_DV_EXP & 3)) {
          bf16x8_t bfr[CJ];
          load_b(le1, t, base, bfr);
#pragma unroll
          for (int i = 0; i < CI; ++i) {
            const bf16x8_t af = a_frag(base, i);
#pragma unroll
            for (int j = 0; j < CJ; ++j) dacc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[j], dacc[i][j], 0, 0, 0);
          }
        }
        dv_signal(&fl_done[slot][NR + c], gen);
        if (++slot == NSL) {
          slot = 0;
          ++gen;
        }
      }
      DV_ACC(3, tl0);
    };
    if (bal <= 1.f) run(std::true_type{});
    else run(std::false_type{});
    DV_STAMP_STORE;
    // dW2 partial of this workgroup: lane holds D[(wp*CI+i)*16 + 4lg + e][n0 + (wn*CJ+j)*16 + lr]
    float* Dp = p.Dpart + (size_t)rr * KR * p.Nout;
#pragma unroll
    for (int i = 0; i < CI; ++i)
#pragma unroll
      for (int j = 0; j < CJ; ++j) {
        const int n = n0 + (wn * CJ + j) * 16 + lr;
#pragma unroll
        // nontemporal for gLN (c2, c5: keeps the activations of the next kernels in the
        // Infinity Cache); plain for cLN: at c4 every tensor is larger than the cache and
        // the hinted dword stores measured 10 us slower per launch (547.7 / 533.6 against
        // 555.3 / 544.7 us, microbenchmark, round 6) — the c4 regression of round 5
        for (int e = 0; e < 4; ++e)
          st_part<NK == NORM_GLN>(&Dp[(size_t)((wp * CI + i) * 16 + 4 * lg + e) * p.Nout + n], dacc[i][j][e]);
      }
    return;
  }

  // ======================= memory waves =======================
  dv_prio<DV_PRIO_MEM, NK>();
  // Memory wave m moves, per tile, A blocks 4m..4m+3 (16 rows x 32 channels of gy each),
  // raw-d pieces 2m, 2m+1 (4 rows x the slice's 128 channels each) and its statistics
  // piece by LDS-DMA (buffer_load ... lds: no registers, PF tiles ahead), waits for its
  // own DMA group with a counted vmcnt (no other memory operations are issued by these
  // waves) and publishes FULL.  A slot is refilled only after every row / column wave's
  // DONE for the tile that used it last.  The raw-d pieces land in the B image itself and
  // wave 0 alone fetches the tile's statistics (all 32 rows).
  const int mw = wid - ND;
  DV_STAMP_DECL;
  const rsrc_t rA = du_rsrc(p.A, rows * p.lda * 2), rD = du_rsrc(p.Bm, rows * p.ldb * 2);
  const rsrc_t rS = du_rsrc(p.bop.stats, (NK == NORM_GLN ? (long)p.g.M : rows) * 8);
  int arow[4];
  uint32_t aoff[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {   // lane L lands at block + 16 L: the fragment-order image
    const int f = 4 * mw + u, mb = f / KB, kb = f % KB;
    arow[u] = 16 * mb + ((lane & 15) ^ (((lane >> 4) & 1) * 12));
    aoff[u] = (uint32_t)(arow[u] * p.lda + (4 * kb + (lane >> 4)) * 8) * 2u;
  }
  // raw-d piece i = 2*mw + h: row 4i + L/16, granule position L%16 holds channels
  // 8g .. 8g+7 with g the granule at B position L%16 (dv_rbpos inverted), the swizzle
  // applied on the source
  uint32_t doff[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int drow = 4 * (2 * mw + h) + (lane >> 4);
    const int ps = lane & 15;
    const int dgr = (ps & 1) | ((((ps >> 1) ^ dv_rbhash(drow)) & 7) << 1);
    doff[h] = (uint32_t)(drow * p.ldb + n0 + 8 * dgr) * 2u;
  }
  // statistics: wave 0 fetches the tile's (cLN: 32 rows, one dword per lane; gLN: the
  // utterance pair, lanes 0..1).  Other lanes read out of range (zeros).
  const bool st_lane = NK == NORM_CLN || lane < 2;
  const uint32_t soff = st_lane ? (uint32_t)(lane * 4) : DU_OOB;
  const bool st_wave = mw == 0;
  const float bal = p.bop.alpha[0];
  // DMA instructions per wave and tile: 7 (st_wave), else 6 (waves 1..3)

  auto dma = [&](int t) __attribute__((always_inline)) {
    if constexpr (CTN_DV_EXP & 32) return;
    char* base = smem + ((t - t0) % NSL) * SLOT;
    const int tk = (t * TM) % Kp;
#pragma unroll
    for (int u = 0; u < 4; ++u)   // rows of padded frames arrive as zeros (out-of-range offset)
      du_dma16(rA, base + OFF_A + (4 * mw + u) * 1024, tk + arow[u] < Kv ? aoff[u] : DU_OOB, t * TM * p.lda * 2);
#pragma unroll
    for (int h = 0; h < 2; ++h) du_dma16(rD, base + OFF_B + (2 * mw + h) * 1024, doff[h], t * TM * p.ldb * 2);
    if (st_wave) du_dma4(rS, base + OFF_ST, soff, NK == NORM_GLN ? (t / tpu) * 8 : t * TM * 8);
  };
  auto run = [&](auto) __attribute__((always_inline)) {
    for (int i = 0; i < PF; ++i)
      if (t0 + i < t1) dma(t0 + i);
    int slot = 0;
    uint32_t gen = 1;
    DV_TS(tl0);
    for (int t = t0; t < t1; ++t) {
      const int later = t1 - 1 - t < PF - 1 ? t1 - 1 - t : PF - 1;   // DMA groups issued after tile t's
      // tile t's DMA group done: every group issued after it may stay in flight (steady
      // state: PF - 1 of them, a compile-time count; the tail waits for all)
      DV_TS(tv0);
      if (later == PF - 1) {
        if (st_wave) dv_vmwait_c<7 * (PF - 1)>();
        else dv_vmwait_c<6 * (PF - 1)>();
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      DV_ACC(1, tv0);
      dv_signal(&fl_full[slot][mw], gen);
      const int tn = t + PF;
      if (tn < t1) {
        const int kn = tn - t0;   // its slot was last used by tile tn - NSL: wait for every DONE of it
        DV_TS(td0);
        dv_wait<ND>(fl_done[kn % NSL], (uint32_t)(kn / NSL), p.err);
        DV_ACC(2, td0);
        dma(tn);
      }
      if (++slot == NSL) {
        slot = 0;
        ++gen;
      }
    }
    DV_ACC(3, tl0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA may land after the wave ends
  };
  // (the loop no longer depends on alpha; the two copies are what the shipped kernel holds,
  // and folding them changes its code and register counts: not part of a pure deletion)
  if (t0 < t1) {
    if (bal <= 1.f) run(std::true_type{});
    else run(std::false_type{});
  }
  DV_STAMP_STORE;
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// CTN_GEMM_DUAL bit 0 (default 1): pair A runs as this one kernel; cleared, as the row GEMM
// + column GEMM kernels (109 us against 62 + 60 us at the time of the choice).
// Every other bit is ignored.  Read on every query so a process can compare both paths
// (tests/test_gpu_tblock.py).  Shapes that are not eligible take the two kernels as well.
bool gemm_dual_eligible(DType dt, const GemmDual& p) {
  const char* e = getenv("CTN_GEMM_DUAL");
  if (dt != BF16 || (e && !(atoi(e) & 1))) return false;
  // Only the paper's 256 -> 512 pair (S = 4 slices) takes the kernel: it is the one shape it is
  // tested and measured at.  The kernel's own arithmetic would admit any Nout that is a multiple
  // of 128 with 256 % S == 0; other widths run the row + column kernels.
  if (!(p.Kred == DV_KR && p.Nout == 512 && p.epi == EPI_NORM_BWD && p.bop.kind == OP_PRELU_NORM)) return false;
  if (p.norm != NORM_GLN && p.norm != NORM_CLN) return false;
  // one final statistics table serves the epilogue and the column operand
  if (p.bop.norm != p.norm || p.stats != p.bop.stats || p.bop.fold.slab) return false;
  if (p.g.Kp % DV_TM || p.lda % 8 || p.ldb % 8 || p.ldc % 8 || p.ldw % 8) return false;
  if (p.g.rows() / DV_TM < 1) return false;
  // 32-bit tile offsets and buffer sizes (du_rsrc clamps at 2^31 bytes)
  if (p.g.rows() * (p.Kred > p.Nout ? p.Kred : p.Nout) * 2 >= (1L << 31)) return false;
  static_assert(512 % DV_NS == 0 && DV_GRID % (512 / DV_NS) == 0, "whole slices, whole row ranges");
  return true;
}

// Row ranges of a launch: the grid is ranges * (Nout / 128) workgroups
int gemm_dual_ranges(const GemmDual& p) {
  const long nt = p.g.rows() / DV_TM;
  const int want = DV_GRID / (p.Nout / DV_NS);
  return (int)(nt < want ? nt : want);
}

// gLN: the run layout of the statistics partials (one run list per range, slice and row wave)
static WsRuns gemm_dual_runs(const GemmDual& p) {
  WsRuns w;
  w.ntile = (int)(p.g.rows() / DV_TM);
  w.grid = gemm_dual_ranges(p);
  w.tpu = p.g.Kp / DV_TM;
  w.waves = p.Nout / DV_NS * DV_NR;
  w.kmax = ws_runs_kmax(w.ntile, w.grid, w.tpu);
  return w;
}

int gemm_dual_group_parts(const GemmDual& p) {
  if (p.norm != NORM_GLN) return p.Nout / DV_NS * DV_CLN_PARTS;
  const WsRuns w = gemm_dual_runs(p);
  const long entries = (long)w.grid * w.waves * w.kmax;
  return (int)((entries + p.g.M - 1) / p.g.M);
}

StatFold gemm_dual_stat_fold(const GemmDual& p, const double2* slab, double cnt, float eps, int mode, float2* out) {
  StatFold f;
  f.slab = slab;
  f.parts = gemm_dual_group_parts(p);
  f.cnt = cnt;
  f.eps = eps;
  f.mode = mode;
  f.out = out;
  if (p.norm == NORM_GLN) f.ws = gemm_dual_runs(p);
  return f;
}

hipError_t launch_gemm_dual(const GemmDual& pa, hipStream_t s) {
  if (!gemm_dual_eligible(BF16, pa)) return hipErrorInvalidValue;
  GemmDual p = pa;
  p.err = device_error_word();
  const dim3 grid(gemm_dual_ranges(p) * (p.Nout / DV_NS));
  if (p.norm == NORM_GLN)
    hipLaunchKernelGGL((gemm_dual_ws_kernel<NORM_GLN, DV_NSL, DV_PF>), grid, dim3(DV_NT), 0, s, p);
  else
    hipLaunchKernelGGL((gemm_dual_ws_kernel<NORM_CLN, DV_NSL, DV_PF>), grid, dim3(DV_NT), 0, s, p);
  return hipGetLastError();
}

}  // namespace ctn
