// STOI and ESTOI (stoi.py, pystoi's algorithm) for a padded batch on the device:
// include/ctn.h ctn_stoi_eval, DESIGN.md §25.  Six kernels on one stream:
//   stoi_resample_kernel  polyphase FIR to 10 kHz, one output sample per lane, fp64 rows
//   stoi_energy_kernel    2-norm of every windowed reference frame, one wave per frame
//   stoi_compact_kernel   keep mask (40 dB below the loudest frame) and its compaction,
//                         one workgroup per reference: idx[] and kept
//   stoi_spectra_kernel   one workgroup per (signal, reference, kept frame): the frame of the
//                         rebuilt signals from three kept frames, x + i y through one complex
//                         512-point FFT in LDS, third-octave band envelopes X, Y
//   stoi_segment_kernel   one wave per four 30-frame segments of a pair: STOI and ESTOI sums
//   stoi_final_kernel     one lane per pair: the segments' sums in index order -> score
// All arithmetic is fp64, every sum has a fixed order and nothing is atomic, so two calls give
// the same bits; no kernel evaluates a trigonometric function (window, twiddles and filter
// come from the caller's table).  Products and sums are not contracted, so that the resampler
// and the overlap-add are the host restatement's operations one for one.
#include "ctn_stoi.h"

#pragma clang fp contract(off)

namespace ctn {

namespace {

constexpr double kStoiEps = 2.220446049250313e-16;         // np.finfo(float).eps
constexpr double kStoiClip = 6.623413251903491;            // 1 + 10^(15 / 20)
constexpr double kStoiShort = 1e-5;                        // fewer than 30 kept frames

// rfft bins [lo, hi) of the 15 third-octave bands from 150 Hz at 10 kHz / 512 (stoi.thirdoct)
__device__ const int kBandLo[STOI_BANDS] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__device__ const int kBandHi[STOI_BANDS] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};
constexpr int kBinLo = 7, kBinHi = 219;

__device__ __forceinline__ int stoi_len(const StoiArgs& a, int m) {
  const int n = a.lengths[m];
  return n < 0 ? 0 : (n > a.T ? a.T : n);
}
__device__ __forceinline__ long stoi_n10(const StoiArgs& a, int len) {
  return ((long)len * a.up + a.down - 1) / a.down;
}
__device__ __forceinline__ int stoi_frames(long n10) {
  return n10 < STOI_FRAME ? 0 : (int)((n10 - STOI_FRAME) / STOI_HOP) + 1;
}

}  // namespace

// ---------------------------------------------------------------------------
// out[k] = sum_i hh[k down - i up + Hl] x[i], i ascending inside the signal; 1/1 copies.
// grid (ceil(n10max / 256), rows per utterance, M); samples past the row's own resampled
// length are written as zeros (no later kernel reads them).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_resample_kernel(StoiArgs a, const float* src, int rows, double* dst) {
  const int m = blockIdx.z, r = blockIdx.y;
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.L.n10max) return;
  const int len = stoi_len(a, m);
  const long n10 = stoi_n10(a, len);
  const float* x = src + ((size_t)m * rows + r) * (size_t)a.T;
  double acc = 0.0;
  if (k < n10) {
    if (a.up == a.down) {
      acc = (double)x[k];
    } else {
      const long c = k * a.down;
      long i0 = c - a.Hl;
      i0 = i0 <= 0 ? 0 : (i0 + a.up - 1) / a.up;
      long i1 = (c + a.Hl) / a.up;
      if (i1 > len - 1) i1 = len - 1;
      const double* hh = a.tab + STOI_TAB_FILTER + a.Hl;
      for (long i = i0; i <= i1; ++i) acc += hh[c - i * a.up] * (double)x[i];
    }
  }
  dst[((size_t)m * rows + r) * (size_t)a.L.n10max + k] = acc;
}

// ---------------------------------------------------------------------------
// nrm[m][c][k] = |w * x[128 k : 128 k + 256]|_2.  One wave per frame, four per workgroup:
// a lane squares its four samples in ascending order, the wave adds in a fixed butterfly.
// grid (ceil(Kmax / 4), C, M)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_energy_kernel(StoiArgs a) {
  const int m = blockIdx.z, c = blockIdx.y, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int K = stoi_frames(stoi_n10(a, stoi_len(a, m)));
  if (k >= K) return;
  const size_t row = (size_t)m * a.C + c;
  const double* x = reinterpret_cast<const double*>(a.ws + a.L.off_ref) + row * (size_t)a.L.n10max +
                    (size_t)STOI_HOP * k;
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double v = a.tab[lane + 64 * q] * x[lane + 64 * q];
    acc += v * v;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
  if (lane == 0) reinterpret_cast<double*>(a.ws + a.L.off_nrm)[row * a.L.Kmax + k] = sqrt(acc);
}

// ---------------------------------------------------------------------------
// Frame k of reference (m, c) is kept iff max(e) - 40 - e_k < 0 with e = 20 log10(nrm + EPS),
// taken in the linear domain: (nrm_k + EPS) * 100 > nrm_max + EPS.  The kept frame numbers
// are compacted by an exclusive prefix sum over chunks of 256 frames with a carried offset.
// grid (C, M), 256 threads
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(STOI_CHUNK) void stoi_compact_kernel(StoiArgs a) {
  __shared__ double smax[STOI_CHUNK];
  __shared__ int scan[STOI_CHUNK];
  __shared__ int carry;
  const int m = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int K = stoi_frames(stoi_n10(a, stoi_len(a, m)));
  const size_t row = (size_t)m * a.C + c;
  const double* nrm = reinterpret_cast<const double*>(a.ws + a.L.off_nrm) + row * a.L.Kmax;
  int32_t* idx = reinterpret_cast<int32_t*>(a.ws + a.L.off_idx) + row * a.L.Kmax;
  double mx = 0.0;
  for (int k = tid; k < K; k += STOI_CHUNK) mx = fmax(mx, nrm[k]);
  smax[tid] = mx;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int off = STOI_CHUNK / 2; off >= 1; off >>= 1) {
    if (tid < off) smax[tid] = fmax(smax[tid], smax[tid + off]);
    __syncthreads();
  }
  const double thr = smax[0] + kStoiEps;
  for (int base = 0; base < K; base += STOI_CHUNK) {
    const int k = base + tid;
    const int flag = (k < K && (nrm[k] + kStoiEps) * 100.0 > thr) ? 1 : 0;
    scan[tid] = flag;
    __syncthreads();
    for (int off = 1; off < STOI_CHUNK; off <<= 1) {
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int before = carry;
    if (flag) idx[before + scan[tid] - 1] = k;
    __syncthreads();
    if (tid == 0) carry = before + scan[STOI_CHUNK - 1];
    __syncthreads();
  }
  if (tid == 0) a.kept[row] = carry;
}

// ---------------------------------------------------------------------------
// Frame j of the rebuilt signals z (the overlap-add of the kept windowed frames at hop 128,
// never stored): z[128 j + n] = w[n + 128] s[128 idx[j-1] + n + 128] + w[n] s[128 idx[j] + n]
// for n < 128 and w[n] s[128 idx[j] + n] + w[n - 128] s[128 idx[j+1] + n - 128] above, added
// in that order (the host's, j ascending).  The windowed frames of x and y go through one
// complex 512-point FFT as x + i y: nine radix-2 decimation-in-frequency stages in LDS
// (8 KB), one butterfly per lane and stage, results in bit-reversed places.  The two
// spectra are split by conjugate symmetry on the bins 7 ... 218 the bands use; a frame that
// is zero in every sample gets zero envelopes without the split.
// LDS banking (ds_read_b64: 32 lanes per cycle over 64 four-byte banks): the stages with a
// half size of 32 and more read and write 32 consecutive doubles per lane group, free of
// conflicts; the five last stages (half size 16 ... 1) touch 32 doubles spread over 64, a
// two-way conflict each.
// grid (Kmax * C, E, M), 256 threads
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stoi_spectra_kernel(StoiArgs a) {
  __shared__ double re[STOI_NFFT], im[STOI_NFFT];
  __shared__ double px[STOI_FRAME], py[STOI_FRAME];
  const int m = blockIdx.z, e = blockIdx.y, c = blockIdx.x % a.C, j = blockIdx.x / a.C, n = threadIdx.x;
  const size_t row = (size_t)m * a.C + c;
  const int Kk = a.kept[row];
  if (j >= Kk) return;
  const int32_t* id = reinterpret_cast<const int32_t*>(a.ws + a.L.off_idx) + row * a.L.Kmax;
  const double* x = reinterpret_cast<const double*>(a.ws + a.L.off_ref) + row * (size_t)a.L.n10max;
  const double* y = reinterpret_cast<const double*>(a.ws + a.L.off_sig) +
                    ((size_t)m * a.E + e) * (size_t)a.L.n10max;
  const double* w = a.tab;
  const double* tw = a.tab + STOI_FRAME;
  double zx = 0.0, zy = 0.0;
  if (n < STOI_HOP) {
    if (j > 0) {
      const size_t o = (size_t)STOI_HOP * id[j - 1] + n + STOI_HOP;
      zx = zx + w[n + STOI_HOP] * x[o];
      zy = zy + w[n + STOI_HOP] * y[o];
    }
    const size_t o = (size_t)STOI_HOP * id[j] + n;
    zx = zx + w[n] * x[o];
    zy = zy + w[n] * y[o];
  } else {
    const size_t o = (size_t)STOI_HOP * id[j] + n;
    zx = zx + w[n] * x[o];
    zy = zy + w[n] * y[o];
    if (j + 1 < Kk) {
      const size_t o2 = (size_t)STOI_HOP * id[j + 1] + n - STOI_HOP;
      zx = zx + w[n - STOI_HOP] * x[o2];
      zy = zy + w[n - STOI_HOP] * y[o2];
    }
  }
  re[n] = w[n] * zx;
  im[n] = w[n] * zy;
  // An all-zero frame has exactly zero envelopes, as on the host; through the shared FFT it
  // would get the other signal's rounding residue, which the scale-invariant scores amplify.
  const int any_x = __syncthreads_or(re[n] != 0.0), any_y = __syncthreads_or(im[n] != 0.0);
  re[n + STOI_FRAME] = 0.0;
  im[n + STOI_FRAME] = 0.0;
  for (int s = 0; s < 9; ++s) {
    __syncthreads();
    const int h = 256 >> s, pos = n & (h - 1);
    const int i0 = ((n - pos) << 1) + pos, i1 = i0 + h;
    const double wr = tw[2 * (pos << s)], wi = tw[2 * (pos << s) + 1];
    const double ar = re[i0], ai = im[i0], br = re[i1], bi = im[i1];
    re[i0] = ar + br;
    im[i0] = ai + bi;
    const double dr = ar - br, di = ai - bi;
    re[i1] = dr * wr - di * wi;
    im[i1] = dr * wi + di * wr;
  }
  __syncthreads();
  if (n >= kBinLo && n < kBinHi) {
    const int p = (int)(__brev((unsigned)n) >> 23), q = (int)(__brev((unsigned)(STOI_NFFT - n)) >> 23);
    const double ar = re[p], ai = im[p], br = re[q], bi = im[q];
    const double xr = 0.5 * (ar + br), xi = 0.5 * (ai - bi);      // X[k] = (Z[k] + conj Z[N-k]) / 2
    const double yr = 0.5 * (ai + bi), yi = 0.5 * (br - ar);      // Y[k] = (Z[k] - conj Z[N-k]) / 2i
    px[n] = any_x ? xr * xr + xi * xi : 0.0;
    py[n] = any_y ? yr * yr + yi * yi : 0.0;
  }
  __syncthreads();
  if (n < 2 * STOI_BANDS) {
    const int b = n % STOI_BANDS, which = n / STOI_BANDS;
    const double* p = which ? py : px;
    double acc = 0.0;
    for (int k = kBandLo[b]; k < kBandHi[b]; ++k) acc += p[k];
    const size_t pair = ((size_t)m * a.E + e) * a.C + c;
    reinterpret_cast<double*>(a.ws + a.L.off_xy)[((pair * a.L.Kmax + j) * 2 + which) * STOI_BANDS + b] = sqrt(acc);
  }
}

// ---------------------------------------------------------------------------
// Segment s of a pair: xs, ys = X, Y[:, s : s + 30].  A wave holds four segments of one
// pair.  Lane 15 g + b owns band b of segment g: the STOI term of the band (scale, clip, mean,
// norm, correlation) and the band's rows of ESTOI (mean / norm along the frames); the 120
// (segment, frame) columns are then normalised along the bands, two passes of the wave, each
// adding its 15 products; lane g adds the bands and the frames of segment g in index order.
// grid (ceil(Jmax / 4) * C, E, M), 64 threads
// ---------------------------------------------------------------------------
__device__ __forceinline__ void stoi_unit(double (&v)[STOI_SEG]) {   // (v - mean) / (|v - mean| + EPS)
  double sum = 0.0;
#pragma unroll
  for (int f = 0; f < STOI_SEG; ++f) sum += v[f];
  const double mean = sum / STOI_SEG;
  double ss = 0.0;
#pragma unroll
  for (int f = 0; f < STOI_SEG; ++f) {
    v[f] = v[f] - mean;
    ss += v[f] * v[f];
  }
  const double den = sqrt(ss) + kStoiEps;
#pragma unroll
  for (int f = 0; f < STOI_SEG; ++f) v[f] = v[f] / den;
}

__global__ __launch_bounds__(64) void stoi_segment_kernel(StoiArgs a) {
  constexpr int G = STOI_SEG_PER_WAVE;
  __shared__ double xn[G][STOI_BANDS][STOI_SEG + 1], yn[G][STOI_BANDS][STOI_SEG + 1];
  __shared__ double dband[G][STOI_BANDS], dframe[G][STOI_SEG];
  const int m = blockIdx.z, e = blockIdx.y, c = blockIdx.x % a.C, s0 = (blockIdx.x / a.C) * G, lane = threadIdx.x;
  const int J = a.kept[(size_t)m * a.C + c] - (STOI_SEG - 1);
  if (s0 >= J) return;
  const size_t pair = ((size_t)m * a.E + e) * a.C + c;
  const int g = lane / STOI_BANDS, band = lane - g * STOI_BANDS;
  if (g < G && s0 + g < J) {
    const double* xy = reinterpret_cast<const double*>(a.ws + a.L.off_xy) +
                       (pair * a.L.Kmax + s0 + g) * (2 * STOI_BANDS) + band;
    double xs[STOI_SEG], ys[STOI_SEG], yp[STOI_SEG];
    double nx = 0.0, ny = 0.0;
#pragma unroll
    for (int f = 0; f < STOI_SEG; ++f) {
      xs[f] = xy[(size_t)f * 2 * STOI_BANDS];
      ys[f] = xy[(size_t)f * 2 * STOI_BANDS + STOI_BANDS];
      nx += xs[f] * xs[f];
      ny += ys[f] * ys[f];
    }
    const double scale = sqrt(nx) / (sqrt(ny) + kStoiEps);
#pragma unroll
    for (int f = 0; f < STOI_SEG; ++f) yp[f] = fmin(ys[f] * scale, xs[f] * kStoiClip);
    stoi_unit(yp);
    stoi_unit(xs);
    stoi_unit(ys);
    double d = 0.0;
#pragma unroll
    for (int f = 0; f < STOI_SEG; ++f) {
      d += yp[f] * xs[f];
      xn[g][band][f] = xs[f];
      yn[g][band][f] = ys[f];
    }
    dband[g][band] = d;
  }
  __syncthreads();
  for (int item = lane; item < G * STOI_SEG; item += 64) {
    const int gg = item / STOI_SEG, f = item - gg * STOI_SEG;
    if (s0 + gg >= J) continue;
    double sx = 0.0, sy = 0.0;
    for (int b = 0; b < STOI_BANDS; ++b) {
      sx += xn[gg][b][f];
      sy += yn[gg][b][f];
    }
    const double mx = sx / STOI_BANDS, my = sy / STOI_BANDS;
    double qx = 0.0, qy = 0.0;
    for (int b = 0; b < STOI_BANDS; ++b) {
      const double u = xn[gg][b][f] - mx, v = yn[gg][b][f] - my;
      qx += u * u;
      qy += v * v;
    }
    const double dx = sqrt(qx) + kStoiEps, dy = sqrt(qy) + kStoiEps;
    double d = 0.0;
    for (int b = 0; b < STOI_BANDS; ++b) {
      const double u = (xn[gg][b][f] - mx) / dx, v = (yn[gg][b][f] - my) / dy;
      d += (u * v) / STOI_SEG;
    }
    dframe[gg][f] = d;
  }
  __syncthreads();
  if (lane < G && s0 + lane < J) {
    double d = 0.0, de = 0.0;
    for (int b = 0; b < STOI_BANDS; ++b) d += dband[lane][b];
    for (int f = 0; f < STOI_SEG; ++f) de += dframe[lane][f];
    double* part = reinterpret_cast<double*>(a.ws + a.L.off_part) + (pair * a.L.Jmax + s0 + lane) * 2;
    part[0] = d;
    part[1] = de;
  }
}

// ---------------------------------------------------------------------------
// score[m][e][c] = { sum_s part[s][0] / (15 J), sum_s part[s][1] / J }, J = kept - 29, the
// sums in index order; kept < 30: 1e-5 twice and status 1.  One lane per pair.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void stoi_final_kernel(StoiArgs a) {
  const size_t pair = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (pair >= (size_t)a.M * a.E * a.C) return;
  const int c = (int)(pair % a.C), e = (int)((pair / a.C) % a.E);
  const size_t m = pair / ((size_t)a.C * a.E);
  const int Kk = a.kept[m * a.C + c];
  const int J = Kk - (STOI_SEG - 1);
  double d = kStoiShort, de = kStoiShort;
  if (J >= 1) {
    const double* part = reinterpret_cast<const double*>(a.ws + a.L.off_part) + pair * a.L.Jmax * 2;
    double sd = 0.0, se = 0.0;
    for (int s = 0; s < J; ++s) {
      sd += part[2 * s];
      se += part[2 * s + 1];
    }
    d = sd / (double)(STOI_BANDS * (long)J);
    de = se / (double)J;
  }
  a.score[pair * 2] = d;
  a.score[pair * 2 + 1] = de;
  if (e == 0) a.status[m * a.C + c] = J >= 1 ? 0 : 1;
}

// ---------------------------------------------------------------------------
StoiLayout stoi_layout(int M, int C, int E, int T, int up, int down) {
  StoiLayout L{};
  L.n10max = ((long)T * up + down - 1) / down;
  L.Kmax = L.n10max < STOI_FRAME ? 0 : (int)((L.n10max - STOI_FRAME) / STOI_HOP) + 1;
  L.Jmax = L.Kmax < STOI_SEG ? 0 : L.Kmax - (STOI_SEG - 1);
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    const size_t at = off;
    off += bytes;
    return at;
  };
  const size_t refs = (size_t)M * C, sigs = (size_t)M * E, pairs = (size_t)M * E * C;
  L.off_ref = take(refs * L.n10max * sizeof(double));
  L.off_sig = take(sigs * L.n10max * sizeof(double));
  L.off_nrm = take(refs * L.Kmax * sizeof(double));
  L.off_idx = take(refs * L.Kmax * sizeof(int32_t));
  L.off_xy = take(pairs * L.Kmax * 2 * STOI_BANDS * sizeof(double));
  L.off_part = take(pairs * L.Jmax * 2 * sizeof(double));
  L.bytes = (off + 255) & ~(size_t)255;
  return L;
}

hipError_t launch_stoi_eval(const StoiArgs& a, hipStream_t s) {
  const unsigned xb = (unsigned)((a.L.n10max + 255) / 256);
  double* ref = reinterpret_cast<double*>(a.ws + a.L.off_ref);
  double* sig = reinterpret_cast<double*>(a.ws + a.L.off_sig);
  stoi_resample_kernel<<<dim3(xb, a.C, a.M), dim3(256), 0, s>>>(a, a.refs, a.C, ref);
  stoi_resample_kernel<<<dim3(xb, a.E, a.M), dim3(256), 0, s>>>(a, a.sigs, a.E, sig);
  if (a.L.Kmax > 0) stoi_energy_kernel<<<dim3((a.L.Kmax + 3) / 4, a.C, a.M), dim3(256), 0, s>>>(a);
  stoi_compact_kernel<<<dim3(a.C, a.M), dim3(STOI_CHUNK), 0, s>>>(a);
  if (a.L.Kmax > 0)
    stoi_spectra_kernel<<<dim3((unsigned)a.L.Kmax * a.C, a.E, a.M), dim3(256), 0, s>>>(a);
  if (a.L.Jmax > 0)
    stoi_segment_kernel<<<dim3((unsigned)((a.L.Jmax + STOI_SEG_PER_WAVE - 1) / STOI_SEG_PER_WAVE) * a.C, a.E, a.M),
                          dim3(64), 0, s>>>(a);
  const size_t pairs = (size_t)a.M * a.E * a.C;
  stoi_final_kernel<<<dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace ctn
