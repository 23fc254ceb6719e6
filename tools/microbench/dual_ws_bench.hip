// Pair-A dual GEMM (ctn_dual_ws.hip) at the paper shapes:
//   * run-to-run reproducibility (every byte of C and of the dW2 partials, and the norm-2
//     statistics per group summed from the partials);
//   * time per launch (hipEvents over NIT launches);
//   * the per-role wait stamps (-DCTN_DV_STAMP=1).
// Build with -DCTN_DV_EXP=<bits> for the bound-finding variants (timing only).
// Usage: dual_ws_bench [M] [K] [g|c] [runs].  Not part of the library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../conv-tasnet_amd/csrc/ctn_dual_ws.hip"

using namespace ctn;

// the library's device error word (ctn_capi_core.hip), here one word of this process
uint32_t* ctn::device_error_word() {
  static uint32_t* w = nullptr;
  if (!w && hipMalloc(&w, 4) == hipSuccess) (void)hipMemset(w, 0, 4);
  return w;
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

static void* dev_fill(size_t bytes, unsigned seed) {
  std::vector<uint16_t> h(bytes / 2);
  unsigned x = seed;
  for (auto& v : h) { x = x * 1664525u + 1013904223u; v = (uint16_t)(0x3c00 + ((x >> 16) & 0x3ff)) ^ ((x >> 8) & 0x8000); }
  void* d; CK(hipMalloc(&d, bytes)); CK(hipMemcpy(d, h.data(), bytes, hipMemcpyHostToDevice));
  return d;
}
template <typename T> static std::vector<T> get(const void* d, size_t n) {
  std::vector<T> h(n);
  CK(hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return h;
}

int main(int argc, char** argv) {
  const int M = argc > 1 ? atoi(argv[1]) : 32, K = argc > 2 ? atoi(argv[2]) : 3199;
  const int NK = argc > 3 && argv[3][0] == 'c' ? NORM_CLN : NORM_GLN;
  const int NRUN = argc > 4 ? atoi(argv[4]) : 10;
  const int Kp = (K + 127) / 128 * 128, B = 256, H = 512;
  const long rows = (long)M * Kp;
  void* gy = dev_fill(rows * B * 2, 5);
  void* d = dev_fill(rows * H * 2, 2);
  void* out = dev_fill(rows * H * 2, 3);
  void* w = dev_fill((size_t)B * H * 2, 4);
  // statistics: gLN per utterance, cLN per row (padded rows: not finite, as the forward leaves them)
  const long G = NK == NORM_GLN ? M : rows;
  std::vector<float> hs(2 * G), hg(H), hb(H);
  for (long i = 0; i < G; ++i) {
    const bool pad = NK == NORM_CLN && i % Kp >= K;
    hs[2 * i] = pad ? NAN : 0.1f + 0.01f * (i % 7);
    hs[2 * i + 1] = pad ? INFINITY : 1.3f - 0.02f * (i % 5);
  }
  for (int i = 0; i < H; ++i) { hg[i] = 0.8f + 0.001f * i; hb[i] = 0.1f - 0.0003f * i; }
  float *st, *gm, *bt, *al, *dpart; double2* slab;
  CK(hipMalloc(&st, hs.size() * 4)); CK(hipMemcpy(st, hs.data(), hs.size() * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&gm, H * 4)); CK(hipMemcpy(gm, hg.data(), H * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&bt, H * 4)); CK(hipMemcpy(bt, hb.data(), H * 4, hipMemcpyHostToDevice));
  float a0 = 0.25f; CK(hipMalloc(&al, 4)); CK(hipMemcpy(al, &a0, 4, hipMemcpyHostToDevice));
  const size_t nslab = (size_t)rows * 16 + 65536;
  CK(hipMalloc(&slab, nslab * sizeof(double2)));
  CK(hipMalloc(&dpart, 64L * B * H * 4));

  GemmDual g{}; g.g = Rows{M, K, Kp}; g.Kred = B; g.Nout = H; g.norm = NK;
  g.A = gy; g.lda = B; g.W = w; g.ldw = B; g.C = out; g.ldc = H; g.epi = EPI_NORM_BWD; g.R = d; g.ldr = H;
  g.alpha = al; g.stats = (const float2*)st; g.gamma = gm; g.grp_slab = slab;
  g.Bm = d; g.ldb = H; g.bop.kind = OP_PRELU_NORM; g.bop.norm = NK; g.bop.stats = (const float2*)st;
  g.bop.gamma = gm; g.bop.beta = bt; g.bop.alpha = al; g.Dpart = dpart;
  if (getenv("DB_FRAG")) g.Wf = w;   // timing: the fragment-order load pattern
  const long cn = rows * H;
  const size_t nd = (size_t)gemm_dual_ranges(g) * B * H;

  struct Out { std::vector<uint16_t> c; std::vector<float> dp; std::vector<double> grp_s, grp_q; };
  auto launch_once = [&](Out* o) {
    CK(hipMemset(out, 0, cn * 2));
    CK(hipMemset(dpart, 0, nd * 4));
    CK(hipMemset(slab, 0, nslab * sizeof(double2)));
    CK(launch_gemm_dual(g, 0));
    CK(hipDeviceSynchronize());
    o->c = get<uint16_t>(out, cn);
    o->dp = get<float>(dpart, nd);
    // per-group totals of the statistics partials
    const int parts = gemm_dual_group_parts(g);
    const auto sl = get<double2>(slab, nslab);
    o->grp_s.assign(G, 0.0);
    o->grp_q.assign(G, 0.0);
    if (NK == NORM_GLN) {
      const WsRuns wr = gemm_dual_runs(g);
      for (int m = 0; m < M; ++m) {
        const int blo = ws_block_of_tile(wr, m * wr.tpu), bhi = ws_block_of_tile(wr, (m + 1) * wr.tpu - 1);
        for (int b = blo; b <= bhi; ++b) {
          const int t0 = ws_t0(wr, b);
          if (t0 >= ws_t0(wr, b + 1)) continue;
          for (int wv = 0; wv < wr.waves; ++wv) {
            const double2 v = sl[((size_t)b * wr.waves + wv) * wr.kmax + (m - t0 / wr.tpu)];
            o->grp_s[m] += v.x;
            o->grp_q[m] += v.y;
          }
        }
      }
    } else {
      for (long r = 0; r < rows; ++r)
        for (int i = 0; i < parts; ++i) { o->grp_s[r] += sl[r * parts + i].x; o->grp_q[r] += sl[r * parts + i].y; }
    }
  };

  // run-to-run reproducibility
  Out cur;
  launch_once(&cur);
  int bad = 0;
  for (int r = 0; r < NRUN; ++r) {
    Out o;
    launch_once(&o);
    long n = 0;
    for (long i = 0; i < cn; ++i) n += o.c[i] != cur.c[i];
    for (size_t i = 0; i < nd; ++i) n += memcmp(&o.dp[i], &cur.dp[i], 4) != 0;
    for (long i = 0; i < G; ++i) n += memcmp(&o.grp_s[i], &cur.grp_s[i], 8) != 0 || memcmp(&o.grp_q[i], &cur.grp_q[i], 8) != 0;
    if (n) { ++bad; printf("   run %d: %ld differing outputs\n", r, n); }
  }
  printf("reproducibility: %d of %d launches differ from the first\n", bad, NRUN);

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  const int NIT = 20;
  const double bytes = rows * (B + 2 * H) * 2.0;
  {
    for (int i = 0; i < 3; ++i) CK(launch_gemm_dual(g, 0));
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < NIT; ++i) CK(launch_gemm_dual(g, 0));
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = ms * 1e3 / NIT;
    printf("EXP %d M=%d K=%d %s %8.1f us  %7.0f GB/s (alg. bytes)\n", CTN_DV_EXP, M, K,
           NK == NORM_GLN ? "gLN" : "cLN", us, bytes / us * 1e-3);
  }
#if CTN_DV_STAMP
  {   // per-role wait shares (one more launch, stamps zeroed)
    std::vector<unsigned long long> h(1024 * 16 * 4, 0ull);
    CK(hipMemcpyToSymbol(HIP_SYMBOL(dv_stamps), h.data(), h.size() * 8));
    CK(launch_gemm_dual(g, 0));
    CK(hipDeviceSynchronize());
    CK(hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(dv_stamps), h.size() * 8));
    const int nwg = gemm_dual_ranges(g) * (H / 128);
    const char* role[3] = {"row", "column", "memory"};
    for (int r = 0; r < 3; ++r) {
      double acc[4] = {0, 0, 0, 0};
      int n = 0;
      for (int b = 0; b < nwg; ++b)
        for (int w = 0; w < 16; ++w) {
          const int rr = w < 4 ? 0 : w < 12 ? 1 : 2;
          if (rr != r) continue;
          ++n;
          for (int i = 0; i < 4; ++i) acc[i] += (double)h[((size_t)b * 16 + w) * 4 + i];
        }
      printf("STAMP %-6s loop %8.0f cyc  full-wait %5.1f%%  dma-vmcnt %5.1f%%  done-wait %5.1f%%\n", role[r],
             acc[3] / n, 100 * acc[0] / acc[3], 100 * acc[1] / acc[3], 100 * acc[2] / acc[3]);
    }
  }
#endif
  return 0;
}
