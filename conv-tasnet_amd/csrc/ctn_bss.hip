// BSS Eval v3 bss_eval_sources (SDR / SIR / SAR energies) for a ragged batch (gfx950).
// Same algorithm and definitions as bss_eval.py (_project / _decompose / _criteria); all
// arithmetic fp64, no atomics, every sum in a fixed order (two runs: same bits).  Samples
// at or beyond lengths[m] are never read into a sum (the padding may hold NaN).
//
// bss_corr   : lag correlations in the direct form.  Per utterance, T chunk and job:
//              r_ij[tau] = sum_t s_i[t+tau] s_j[t], tau in (-flen, flen), for every reference
//              pair i <= j, and d_ei[tau] = sum_t sig_e[t+tau] s_i[t], tau in [0, flen), for
//              every (signal, reference).  Both windows staged in LDS as fp64; a thread owns
//              up to four lags and walks t in order.  Per-chunk partials.
// bss_lagsum : partials summed in chunk order; status[m] = 0.
// bss_expand : lags -> block-Toeplitz Gram matrices G[(i,a),(j,b)] = r_ij[b-a] (one of order
//              C*flen, and for C > 1 one of order flen per reference) and the right-hand
//              sides D[(i,a)] = d_ei[a] (bss_eval.py _project; the solution reshaped
//              column-major (flen, nsrc) is x[i*flen + k] = c[k, i]).
// bss_chol_* : blocked right-looking Cholesky of every (utterance, system), L stored so that
//              L[r][c] sits at A[c*n + r] (a column is contiguous).  Per 32-column step three
//              launches over all systems: the diagonal block factored in LDS (one workgroup
//              per system), the panel solve (one row per thread, the row in registers), the
//              trailing update in 64x64 tiles (one per workgroup, 4x4 per thread, the panel
//              rows in LDS).  A pivot that is not finite or <= n * 2^-52 * max diag sets the
//              system's flag and every later launch skips the system.
// bss_solve  : one workgroup per system: forward and backward substitution of all E
//              right-hand sides against the one factor, up to 8 at a time in LDS; a flagged
//              system sets status[m] = 1 instead.
// bss_proj   : per (utterance, signal, 1024-sample tile): p_all[t] = sum_i sum_k c_all[k,i]
//              s_i[t-k] and, per reference j, p_j[t] from j's single-reference filter, taps
//              and reference windows in LDS, t in [0, n + flen - 1); five sums per j:
//              |p_j|^2, |p_all-p_j|^2, |ep-p_j|^2, |p_all|^2, |ep-p_all|^2 (ep = the signal
//              zero-extended).  C == 1: p_j is p_all itself, so |e_interf|^2 is exactly 0.
// bss_energy : per-tile partials summed in tile order.
#include "ctn_bss.h"
#include "ctn_common.h"

namespace ctn {

constexpr int BSS_CH = 2048;    // samples of t per correlation chunk
constexpr int BSS_LG = 1024;    // lags per correlation workgroup (4 per thread)
constexpr int BSS_NB = 32;      // Cholesky panel width
constexpr int BSS_TL = 64;      // trailing-update tile
constexpr int BSS_TT = 1024;    // projection outputs per workgroup (4 per thread)
constexpr int BSS_KB = 256;     // taps staged at a time

BssLayout bss_layout(int M, int C, int E, int T, int flen) {
  BssLayout L{};
  const size_t n = (size_t)C * flen;
  L.NP = C * (C + 1) / 2;
  L.nchunk = (T + BSS_CH - 1) / BSS_CH;
  L.ntile = (T + flen - 1 + BSS_TT - 1) / BSS_TT;
  L.nsys = C > 1 ? C + 1 : 1;
  L.LV = (size_t)L.NP * (2 * flen - 1) + (size_t)E * C * flen;
  L.sys_elems = n * n + (C > 1 ? (size_t)C * flen * flen : 0);
  L.coef_elems = (size_t)E * n * (C > 1 ? 2 : 1);
  size_t o = 0;
  L.off_part = o;  o += (size_t)M * L.nchunk * L.LV;
  L.off_lag = o;   o += (size_t)M * L.LV;
  L.off_gram = o;  o += (size_t)M * L.sys_elems;
  L.off_coef = o;  o += (size_t)M * L.coef_elems;
  L.off_epart = o; o += (size_t)M * E * L.ntile * C * 5;
  L.off_flag = o;  o += ((size_t)M * L.nsys + 1) / 2;      // one int per system
  L.bytes = o * sizeof(double);
  return L;
}

CTN_DEV int bss_len(const BssArgs& a, int m) {
  const int n = a.lengths[m];
  return n < 0 ? 0 : (n > a.T ? a.T : n);
}

// ---------------------------------------------------------------------------
// lag correlations
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bss_corr_kernel(BssArgs a, int gp, int gd) {
  __shared__ double sb[BSS_CH];
  __shared__ double sa[BSS_CH + BSS_LG];
  const int tid = threadIdx.x, chunk = blockIdx.y, m = blockIdx.z;
  const int C = a.C, E = a.E, T = a.T, flen = a.flen;
  const int n = bss_len(a, m);
  const int t0 = chunk * BSS_CH;
  if (t0 >= n) return;                     // bss_lagsum reads only the chunks below the length
  const int nt = (t0 + BSS_CH < n ? t0 + BSS_CH : n) - t0;
  int job = blockIdx.x;
  const int npj = a.L.NP * gp;
  const float *pa, *pb;
  int lag_lo, nlag, g;
  size_t out;
  if (job < npj) {
    int pair = job / gp, i = 0;
    g = job % gp;
    out = (size_t)pair * (2 * flen - 1);
    while (pair >= C - i) { pair -= C - i; ++i; }
    pa = a.refs + ((size_t)m * C + i) * T;
    pb = a.refs + ((size_t)m * C + i + pair) * T;
    lag_lo = -(flen - 1);
    nlag = 2 * flen - 1;
  } else {
    job -= npj;
    const int ei = job / gd;
    g = job % gd;
    out = (size_t)a.L.NP * (2 * flen - 1) + (size_t)ei * flen;
    pa = a.sigs + ((size_t)m * E + ei / C) * T;
    pb = a.refs + ((size_t)m * C + ei % C) * T;
    lag_lo = 0;
    nlag = flen;
  }
  const int l0 = g * BSS_LG;
  const int nl = nlag - l0 < BSS_LG ? nlag - l0 : BSS_LG;
  // sa[w] = a[t0 + lag_lo + l0 + w], w < nt + nl - 1 (<= BSS_CH + BSS_LG - 1)
  const int wbase = t0 + lag_lo + l0;
  for (int w = tid; w < nt + nl - 1; w += 256) {
    const int ta = wbase + w;
    sa[w] = (ta >= 0 && ta < n) ? (double)pa[ta] : 0.0;
  }
  for (int w = tid; w < nt; w += 256) sb[w] = (double)pb[t0 + w];
  __syncthreads();
  int lk[4];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 4; ++k) lk[k] = tid + 256 * k < nl ? tid + 256 * k : nl - 1;
  for (int t = 0; t < nt; ++t) {
    const double b = sb[t];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] += sa[t + lk[k]] * b;
  }
  double* o = a.ws + a.L.off_part + ((size_t)m * a.L.nchunk + chunk) * a.L.LV + out + l0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tid + 256 * k < nl) o[tid + 256 * k] = acc[k];
}

__global__ __launch_bounds__(256) void bss_lagsum_kernel(BssArgs a) {
  const int m = blockIdx.y;
  const size_t l = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (l == 0) a.status[m] = 0;
  if (l < (size_t)a.L.nsys) reinterpret_cast<int*>(a.ws + a.L.off_flag)[(size_t)m * a.L.nsys + l] = 0;
  if (l >= a.L.LV) return;
  const int n = bss_len(a, m);
  const int nch = (n + BSS_CH - 1) / BSS_CH;
  const double* p = a.ws + a.L.off_part + (size_t)m * a.L.nchunk * a.L.LV + l;
  double s = 0.0;
  for (int c = 0; c < nch; ++c) s += p[(size_t)c * a.L.LV];
  a.ws[a.L.off_lag + (size_t)m * a.L.LV + l] = s;
}

// ---------------------------------------------------------------------------
// Gram matrices and right-hand sides
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bss_expand_kernel(BssArgs a) {
  const int m = blockIdx.y;
  const int C = a.C, E = a.E, flen = a.flen, n = C * flen;
  const int nl = 2 * flen - 1;
  const double* lag = a.ws + a.L.off_lag + (size_t)m * a.L.LV;
  const double* dl = lag + (size_t)a.L.NP * nl;           // d_ei[k] at (e*C + i)*flen + k
  double* G = a.ws + a.L.off_gram + (size_t)m * a.L.sys_elems;
  double* cf = a.ws + a.L.off_coef + (size_t)m * a.L.coef_elems;
  const size_t nfull = (size_t)n * n;
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < nfull; idx += stride) {
    const int X = (int)(idx / n), Y = (int)(idx % n);
    int i = X / flen, ia = X % flen, j = Y / flen, jb = Y % flen;
    if (i > j) { int t = i; i = j; j = t; t = ia; ia = jb; jb = t; }
    const size_t pair = (size_t)i * C - (size_t)i * (i - 1) / 2 + (j - i);
    G[idx] = lag[pair * nl + (jb - ia) + flen - 1];
  }
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < (size_t)E * n; idx += stride)
    cf[idx] = dl[idx];                                     // full system: [e][i*flen + k]
  if (C > 1) {
    const size_t ns = (size_t)C * flen * flen;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < ns; idx += stride) {
      const int j = (int)(idx / ((size_t)flen * flen));
      const int r = (int)(idx % ((size_t)flen * flen));
      const size_t pair = (size_t)j * C - (size_t)j * (j - 1) / 2;
      G[nfull + idx] = lag[pair * nl + (r % flen - r / flen) + flen - 1];
    }
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < (size_t)E * n; idx += stride) {
      const int k = (int)(idx % flen), e = (int)((idx / flen) % E), j = (int)(idx / ((size_t)flen * E));
      cf[(size_t)E * n + idx] = dl[((size_t)e * C + j) * flen + k];   // single systems: [j][e][k]
    }
  }
}

// ---------------------------------------------------------------------------
// Cholesky factorisation and the solves
// ---------------------------------------------------------------------------
struct BssSys {
  int n;          // order
  double* A;      // L[r][c] at A[c*n + r]
  double* rhs;    // [E][n]
  int* flag;      // 1: a pivot of this system failed
};

CTN_DEV BssSys bss_sys(const BssArgs& a, int m, int sys) {
  const int nfull = a.C * a.flen;
  BssSys s;
  s.n = sys == 0 ? nfull : a.flen;
  s.A = a.ws + a.L.off_gram + (size_t)m * a.L.sys_elems +
        (sys == 0 ? 0 : (size_t)nfull * nfull + (size_t)(sys - 1) * a.flen * a.flen);
  s.rhs = a.ws + a.L.off_coef + (size_t)m * a.L.coef_elems +
          (sys == 0 ? 0 : (size_t)a.E * nfull + (size_t)(sys - 1) * a.E * a.flen);
  s.flag = reinterpret_cast<int*>(a.ws + a.L.off_flag) + (size_t)m * a.L.nsys + sys;
  return s;
}

CTN_DEV void bss_load_diag(double* sh, const double* A, int n, int k, int nb) {
  for (int idx = threadIdx.x; idx < nb * nb; idx += 256) {
    const int r = idx % nb, c = idx / nb;
    if (r >= c) sh[r * (BSS_NB + 1) + c] = A[(size_t)(k + c) * n + k + r];
  }
}

// step k, part 1: the diagonal block A[k:k+nb, k:k+nb] -> its Cholesky factor (in LDS)
__global__ __launch_bounds__(256) void bss_chol_diag_kernel(BssArgs a, int k) {
  __shared__ double sh[BSS_NB * (BSS_NB + 1)];
  const int tid = threadIdx.x, sys = blockIdx.x, m = blockIdx.y;
  const BssSys S = bss_sys(a, m, sys);
  const int n = S.n;
  if (k >= n || *S.flag) return;
  // largest diagonal entry of the system as built: r_ii[0] of its references
  const double* lag = a.ws + a.L.off_lag + (size_t)m * a.L.LV;
  const int nl = 2 * a.flen - 1;
  double mx = 0.0;
  for (int i = sys == 0 ? 0 : sys - 1; i < (sys == 0 ? a.C : sys); ++i) {
    const double v = lag[((size_t)i * a.C - (size_t)i * (i - 1) / 2) * nl + a.flen - 1];
    if (!(v <= mx)) mx = v;
  }
  const double tol = (double)n * 2.220446049250313e-16 * mx;
  const int nb = n - k < BSS_NB ? n - k : BSS_NB;
  bss_load_diag(sh, S.A, n, k, nb);
  __syncthreads();
  for (int c = 0; c < nb; ++c) {
    const double d = sh[c * (BSS_NB + 1) + c];
    if (!(d > tol) || isinf(d)) {              // the same value in every thread: uniform exit
      if (tid == 0) *S.flag = 1;
      return;
    }
    const double ld = sqrt(d);
    __syncthreads();
    if (tid == 0) sh[c * (BSS_NB + 1) + c] = ld;
    if (tid > c && tid < nb) sh[tid * (BSS_NB + 1) + c] /= ld;
    __syncthreads();
    for (int idx = tid; idx < nb * nb; idx += 256) {
      const int r = idx % nb, q = idx / nb;
      if (q > c && r >= q) sh[r * (BSS_NB + 1) + q] -= sh[r * (BSS_NB + 1) + c] * sh[q * (BSS_NB + 1) + c];
    }
    __syncthreads();
  }
  for (int idx = tid; idx < nb * nb; idx += 256) {
    const int r = idx % nb, c = idx / nb;
    if (r >= c) S.A[(size_t)(k + c) * n + k + r] = sh[r * (BSS_NB + 1) + c];
  }
}

// step k, part 2: the panel below the diagonal block, L21 = A21 L11^-T, one row per thread
__global__ __launch_bounds__(256) void bss_chol_panel_kernel(BssArgs a, int k) {
  __shared__ double sh[BSS_NB * (BSS_NB + 1)];
  const int sys = blockIdx.y, m = blockIdx.z;
  const BssSys S = bss_sys(a, m, sys);
  const int n = S.n;
  const int rb = k + BSS_NB + blockIdx.x * 256;
  if (rb >= n || *S.flag) return;              // rows exist below: the block is a full BSS_NB wide
  bss_load_diag(sh, S.A, n, k, BSS_NB);
  __syncthreads();
  const int r = rb + threadIdx.x;
  if (r >= n) return;
  double x[BSS_NB];
#pragma unroll
  for (int c = 0; c < BSS_NB; ++c) {
    asm volatile("" ::: "memory");              // keep the 528 L11 reads out of registers
    double v = S.A[(size_t)(k + c) * n + r];
#pragma unroll
    for (int p = 0; p < c; ++p) v -= x[p] * sh[c * (BSS_NB + 1) + p];
    x[c] = v / sh[c * (BSS_NB + 1) + c];
    S.A[(size_t)(k + c) * n + r] = x[c];
  }
}

// step k, part 3: trailing update A22 -= L21 L21^T, one 64x64 tile (I >= J) per workgroup
__global__ __launch_bounds__(256) void bss_chol_update_kernel(BssArgs a, int k) {
  __shared__ double LI[BSS_NB * BSS_TL];
  __shared__ double LJ[BSS_NB * BSS_TL];
  const int tid = threadIdx.x, sys = blockIdx.y, m = blockIdx.z;
  const BssSys S = bss_sys(a, m, sys);
  const int n = S.n, r0 = k + BSS_NB;
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
  const int J = (int)blockIdx.x - I * (I + 1) / 2;
  if (r0 + I * BSS_TL >= n || *S.flag) return;
  for (int idx = tid; idx < BSS_NB * BSS_TL; idx += 256) {
    const int p = idx / BSS_TL, ri = r0 + I * BSS_TL + idx % BSS_TL, rj = r0 + J * BSS_TL + idx % BSS_TL;
    LI[idx] = ri < n ? S.A[(size_t)(k + p) * n + ri] : 0.0;
    LJ[idx] = rj < n ? S.A[(size_t)(k + p) * n + rj] : 0.0;
  }
  __syncthreads();
  const int tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
#pragma unroll 4
  for (int p = 0; p < BSS_NB; ++p) {
    double li[4], lj[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      li[u] = LI[p * BSS_TL + tx + 16 * u];
      lj[u] = LJ[p * BSS_TL + ty + 16 * u];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[u][v] += li[u] * lj[v];
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const int cc = r0 + J * BSS_TL + ty + 16 * v;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rr = r0 + I * BSS_TL + tx + 16 * u;
      if (rr < n && cc <= rr) S.A[(size_t)cc * n + rr] -= acc[u][v];
    }
  }
}

// L y = b, L^T x = y: one workgroup per system, up to BSS_RG right-hand sides at a time in LDS
// (thread t: right-hand side t / 32, row t % 32 of the diagonal block)
constexpr int BSS_RG = 8;
__global__ __launch_bounds__(256) void bss_solve_kernel(BssArgs a) {
  __shared__ double sh[BSS_NB * (BSS_NB + 1)];
  __shared__ double vec[BSS_MAX_ORDER];
  const int tid = threadIdx.x, sys = blockIdx.x, m = blockIdx.y;
  const BssSys S = bss_sys(a, m, sys);
  const int n = S.n, E = a.E;
  const double* A = S.A;
  if (*S.flag) {
    if (tid == 0) a.status[m] = 1;
    return;
  }
  const int gmax = BSS_MAX_ORDER / n < BSS_RG ? BSS_MAX_ORDER / n : BSS_RG;
  const int tg = tid >> 5, tr = tid & 31;
  const int klast = ((n - 1) / BSS_NB) * BSS_NB;
  for (int e0 = 0; e0 < E; e0 += gmax) {
    const int G = E - e0 < gmax ? E - e0 : gmax;
    double* b = S.rhs + (size_t)e0 * n;         // G consecutive right-hand sides: vec[g*n + r]
    __syncthreads();
    for (int i = tid; i < G * n; i += 256) vec[i] = b[i];
    for (int k = 0; k < n; k += BSS_NB) {
      const int nb = n - k < BSS_NB ? n - k : BSS_NB;
      __syncthreads();
      bss_load_diag(sh, A, n, k, nb);
      __syncthreads();
      for (int c = 0; c < nb; ++c) {
        if (tr == c && tg < G) vec[tg * n + k + c] /= sh[c * (BSS_NB + 1) + c];
        __syncthreads();
        if (tr > c && tr < nb && tg < G) vec[tg * n + k + tr] -= sh[tr * (BSS_NB + 1) + c] * vec[tg * n + k + c];
        __syncthreads();
      }
      for (int r = k + nb + tid; r < n; r += 256) {
        double s[BSS_RG];
#pragma unroll
        for (int g = 0; g < BSS_RG; ++g) s[g] = 0.0;
        for (int p = 0; p < nb; ++p) {
          const double l = A[(size_t)(k + p) * n + r];
#pragma unroll
          for (int g = 0; g < BSS_RG; ++g)
            if (g < G) s[g] += l * vec[g * n + k + p];
        }
#pragma unroll
        for (int g = 0; g < BSS_RG; ++g)
          if (g < G) vec[g * n + r] -= s[g];
      }
    }
    for (int k = klast; k >= 0; k -= BSS_NB) {
      const int nb = n - k < BSS_NB ? n - k : BSS_NB;
      __syncthreads();
      bss_load_diag(sh, A, n, k, nb);
      __syncthreads();
      for (int c = nb - 1; c >= 0; --c) {
        if (tr == c && tg < G) vec[tg * n + k + c] /= sh[c * (BSS_NB + 1) + c];
        __syncthreads();
        if (tr < c && tg < G) vec[tg * n + k + tr] -= sh[c * (BSS_NB + 1) + tr] * vec[tg * n + k + c];
        __syncthreads();
      }
      for (int c = tid; c < k; c += 256) {
        double s[BSS_RG];
#pragma unroll
        for (int g = 0; g < BSS_RG; ++g) s[g] = 0.0;
        for (int p = 0; p < nb; ++p) {
          const double l = A[(size_t)c * n + k + p];
#pragma unroll
          for (int g = 0; g < BSS_RG; ++g)
            if (g < G) s[g] += l * vec[g * n + k + p];
        }
#pragma unroll
        for (int g = 0; g < BSS_RG; ++g)
          if (g < G) vec[g * n + c] -= s[g];
      }
    }
    __syncthreads();
    for (int i = tid; i < G * n; i += 256) b[i] = vec[i];
  }
}

// ---------------------------------------------------------------------------
// projection and energies
// ---------------------------------------------------------------------------
// acc[q] += sum_k taps[k] * s[t0 + tid + 256 q - k], s read only inside [0, n)
CTN_DEV void bss_filter(double (&acc)[4], const float* s, const double* taps, int flen, int n, int t0, double* win,
                        double* tap) {
  const int tid = threadIdx.x;
  for (int kb = 0; kb < flen; kb += BSS_KB) {
    const int nk = flen - kb < BSS_KB ? flen - kb : BSS_KB;
    __syncthreads();
    if (tid < nk) tap[tid] = taps[kb + tid];
    // win[w] = s[t0 - kb - (BSS_KB - 1) + w], w < BSS_TT + BSS_KB - 1
    for (int w = tid; w < BSS_TT + BSS_KB - 1; w += 256) {
      const int ts = t0 - kb - (BSS_KB - 1) + w;
      win[w] = (ts >= 0 && ts < n) ? (double)s[ts] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      const double c = tap[k];
      const double* wp = win + tid - k + BSS_KB - 1;
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[q] += c * wp[256 * q];
    }
  }
}

__global__ __launch_bounds__(256) void bss_proj_kernel(BssArgs a) {
  __shared__ double win[BSS_TT + BSS_KB];
  __shared__ double tap[BSS_KB];
  __shared__ double red[5 * 4];
  const int tid = threadIdx.x, tile = blockIdx.x, e = blockIdx.y, m = blockIdx.z;
  const int C = a.C, E = a.E, T = a.T, flen = a.flen, nfull = C * flen;
  const int n = bss_len(a, m);
  const int t0 = tile * BSS_TT;
  if (n <= 0 || t0 >= n + flen - 1) return;   // bss_energy reads only the tiles below n + flen - 1
  const double* cf = a.ws + a.L.off_coef + (size_t)m * a.L.coef_elems;
  const double* call = cf + (size_t)e * nfull;
  double pall[4] = {0.0, 0.0, 0.0, 0.0}, ep[4];
  for (int i = 0; i < C; ++i)
    bss_filter(pall, a.refs + ((size_t)m * C + i) * T, call + (size_t)i * flen, flen, n, t0, win, tap);
  double s_all = 0.0, s_art = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int t = t0 + tid + 256 * q;
    ep[q] = t < n ? (double)a.sigs[((size_t)m * E + e) * T + t] : 0.0;
    s_all += pall[q] * pall[q];
    s_art += (ep[q] - pall[q]) * (ep[q] - pall[q]);
  }
  double* out = a.ws + a.L.off_epart + (((size_t)m * E + e) * a.L.ntile + tile) * C * 5;
  for (int j = 0; j < C; ++j) {
    double pj[4] = {0.0, 0.0, 0.0, 0.0};
    if (C == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) pj[q] = pall[q];
    } else {
      bss_filter(pj, a.refs + ((size_t)m * C + j) * T, cf + (size_t)E * nfull + ((size_t)j * E + e) * flen, flen, n,
                 t0, win, tap);
    }
    double v[5] = {0.0, 0.0, 0.0, s_all, s_art};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[0] += pj[q] * pj[q];
      v[1] += (pall[q] - pj[q]) * (pall[q] - pj[q]);
      v[2] += (ep[q] - pj[q]) * (ep[q] - pj[q]);
    }
    if (C == 1) { v[0] = s_all; v[2] = s_art; }     // the same sums: SDR == SAR bit for bit
    block_sum_d<5>(v, red);
    if (tid == 0)
#pragma unroll
      for (int q = 0; q < 5; ++q) out[(size_t)j * 5 + q] = v[q];
  }
}

__global__ __launch_bounds__(256) void bss_energy_kernel(BssArgs a) {
  const int m = blockIdx.y;
  const size_t per = (size_t)a.C * 5;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;      // (e, j, q)
  if (idx >= (size_t)a.E * per) return;
  const int n = bss_len(a, m);
  const int nt = n > 0 ? (n + a.flen - 1 + BSS_TT - 1) / BSS_TT : 0;
  const size_t e = idx / per, jq = idx % per;
  const double* p = a.ws + a.L.off_epart + ((size_t)m * a.E + e) * a.L.ntile * per + jq;
  double s = 0.0;
  for (int t = 0; t < nt; ++t) s += p[(size_t)t * per];
  a.energies[(size_t)m * a.E * per + idx] = s;
}

hipError_t launch_bss_eval(const BssArgs& a, hipStream_t s) {
  const int gp = (2 * a.flen - 1 + BSS_LG - 1) / BSS_LG, gd = (a.flen + BSS_LG - 1) / BSS_LG;
  const unsigned jobs = (unsigned)(a.L.NP * gp + a.E * a.C * gd);
  const size_t n = (size_t)a.C * a.flen;
  bss_corr_kernel<<<dim3(jobs, a.L.nchunk, a.M), 256, 0, s>>>(a, gp, gd);
  bss_lagsum_kernel<<<dim3((unsigned)((a.L.LV + a.L.nsys + 255) / 256), a.M), 256, 0, s>>>(a);
  size_t xb = (n * n + 255) / 256;
  if (xb > 4096) xb = 4096;
  bss_expand_kernel<<<dim3((unsigned)xb, a.M), 256, 0, s>>>(a);
  for (int k = 0; k < (int)n; k += BSS_NB) {
    bss_chol_diag_kernel<<<dim3(a.L.nsys, a.M), 256, 0, s>>>(a, k);
    const int rest = (int)n - k - BSS_NB;
    if (rest <= 0) break;
    const int ntl = (rest + BSS_TL - 1) / BSS_TL;
    bss_chol_panel_kernel<<<dim3((rest + 255) / 256, a.L.nsys, a.M), 256, 0, s>>>(a, k);
    bss_chol_update_kernel<<<dim3(ntl * (ntl + 1) / 2, a.L.nsys, a.M), 256, 0, s>>>(a, k);
  }
  bss_solve_kernel<<<dim3(a.L.nsys, a.M), 256, 0, s>>>(a);
  bss_proj_kernel<<<dim3(a.L.ntile, a.E, a.M), 256, 0, s>>>(a);
  bss_energy_kernel<<<dim3((unsigned)(((size_t)a.E * a.C * 5 + 255) / 256), a.M), 256, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace ctn
