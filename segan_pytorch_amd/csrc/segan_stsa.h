// What the short-time spectral-amplitude enhancers share (segan_denoise.hip: Wiener and log-MMSE,
// DESIGN.md section 20; segan_omlsa.hip: OM-LSA with IMCRA, section 23): the framing, the window
// and twiddle tables, the direct DFT of the analysis, E1, and the overlap-add synthesis.  Each
// enhancer keeps its own recursion kernel between the two.
//
//   denoise_analysis_kernel   one workgroup per (frame, row), one thread per bin: the windowed
//                             frame and the N twiddles in LDS, a direct DFT of the bins 0 .. F in
//                             ascending n into spec [rows][nfmax][F + 1].  Launched with nfmax + 1
//                             workgroups per row, the last one takes the six leading noise frames,
//                             adds |X_j| in ascending j and writes lambda_0 [rows][F + 1]
//                             (section 20); launched with nfmax, lam0 is not touched
//   denoise_synthesis_kernel  one workgroup per (hop, row), one thread per sample: the inverse DFT
//                             of the two frames that cover the hop at the hop's samples only, the
//                             earlier frame added first; zeros from (nf + 1) H on; a row without
//                             frames is copied
//
// Everything is in an unnamed namespace: each of the two files has its own instance of the kernels
// and of the table cache.
#pragma once
#include "segan_signal.h"
#include <float.h>

// the oracles round every product and every sum on their own; the DFT sums ask for their fused
// multiply-adds by name.  In force for the rest of the including file.
#pragma clang fp contract(off)

#define DN_MAX_F 320           // the 16 kHz constants; 8 kHz halves them
#define DN_MAX_T (1 << 24)
#define DN_NOISE_FRAMES 6

namespace {

struct DnRate {
  int F, H, N;
};

__host__ __device__ inline bool dn_rate(int srate, DnRate* d) {
  if (srate != 16000 && srate != 8000) return false;
  d->F = srate / 50;
  d->H = d->F / 2;
  d->N = 2 * d->F;
  return true;
}

// frames of a row of L samples: none below the six noise frames
__host__ __device__ inline int dn_frames(int L, const DnRate& d) {
  return L >= DN_NOISE_FRAMES * d.F ? L / d.H - 1 : 0;
}

struct DnTable {
  int device, srate;
  double* win;     // [F]
  double2* tw;     // [N]: (cos, sin)(2 pi m / N)
};
SeganDeviceTables<DnTable> g_dn_tables;

const DnTable* dn_table(int srate) {
  return g_dn_tables.get(
      "denoise", [srate](const DnTable& e) { return e.srate == srate; },
      [srate](DnTable* e) {
        DnRate d;
        dn_rate(srate, &d);
        std::vector<double> w(d.F);
        double sum = 0.0;
        for (int n = 0; n < d.F; ++n) {
          w[n] = 0.54 - 0.46 * cos(2.0 * M_PI * (double)n / (double)(d.F - 1));
          sum += w[n];
        }
        const double scale = (double)d.H / sum;
        for (int n = 0; n < d.F; ++n) w[n] = w[n] * scale;
        e->srate = srate;
        return segan_upload(&e->win, w, "denoise") &&
               segan_upload(&e->tw, segan_twiddles(d.N), "denoise");
      });
}

__device__ __forceinline__ void dn_load_twiddles(double2* tw, const double2* __restrict__ twg,
                                                 int N) {
  for (int i = threadIdx.x; i < N; i += blockDim.x) tw[i] = twg[i];
}

// bin k of DFT_N of the F samples xs: re = sum xs[n] cos, im = -sum xs[n] sin, n ascending
__device__ __forceinline__ double2 dn_bin(const double* xs, const double2* tw, int k, int F,
                                          int N) {
  double re = 0.0, ims = 0.0;
  int idx = 0;
  for (int n = 0; n < F; ++n) {
    const double2 w = tw[idx];
    const double v = xs[n];
    re = fma(v, w.x, re);
    ims = fma(v, w.y, ims);
    idx += k;
    if (idx >= N) idx -= N;
  }
  return make_double2(re, -ims);
}

template <typename Tin>
__global__ __launch_bounds__(384) void denoise_analysis_kernel(
    const Tin* __restrict__ x, const int* __restrict__ lengths, int T, DnRate dr, int nfmax,
    const double* __restrict__ win, const double2* __restrict__ twg, double2* __restrict__ spec,
    double* __restrict__ lam0) {
  __shared__ double2 tw[2 * DN_MAX_F];
  __shared__ double xs[DN_MAX_F];
  const int r = blockIdx.y, b = blockIdx.x, k = threadIdx.x;
  const int F = dr.F, N = dr.N;
  const int L = segan_row_samples(lengths, r, T);
  const int nf = dn_frames(L, dr);
  if (b < nfmax && b >= nf) return;   // the whole workgroup, before any barrier
  if (nf == 0) return;
  const Tin* xr = x + (size_t)r * T;
  dn_load_twiddles(tw, twg, N);
  if (b < nfmax) {
    // frame b: samples b H .. b H + F - 1 < (nf + 1) H <= L
    const int s0 = b * dr.H;
    for (int n = k; n < F; n += blockDim.x) xs[n] = win[n] * (double)xr[s0 + n];
    __syncthreads();
    if (k <= F) spec[((size_t)r * nfmax + b) * (size_t)(F + 1) + k] = dn_bin(xs, tw, k, F, N);
    return;
  }
  // the six leading frames, 6 F <= L: the mean magnitude in ascending frame order
  double m = 0.0;
  for (int j = 0; j < DN_NOISE_FRAMES; ++j) {
    for (int n = k; n < F; n += blockDim.x) xs[n] = win[n] * (double)xr[j * F + n];
    __syncthreads();
    if (k <= F) {
      const double2 X = dn_bin(xs, tw, k, F, N);
      m += sqrt(X.x * X.x + X.y * X.y);
    }
    __syncthreads();
  }
  if (k <= F) {
    m = m / (double)DN_NOISE_FRAMES;
    lam0[(size_t)r * (F + 1) + k] = fmax(m * m, 0x1p-100);
  }
}

// E1(x), x > 0: the power series below 1, the modified Lentz continued fraction from 1 on, both
// stopped at a relative step of 2^-53 (scripts/denoise_oracle.py: exp1)
__device__ __forceinline__ double dn_exp1(double x) {
  const double step = 0x1p-53;
  if (x < 1.0) {
    double p = 1.0, acc = 0.0;
    for (int n = 1; n <= 100; ++n) {
      p = p * (-x) / (double)n;
      const double term = p / (double)n;
      acc += term;
      if (fabs(term) <= step * fabs(acc)) break;
    }
    return (-0.5772156649015328606065120900824024 - log(x)) - acc;
  }
  double b = x + 1.0, c = DBL_MAX, d = 1.0 / b, h = d;
  for (int i = 1; i <= 400; ++i) {
    const double a = -(double)i * (double)i;
    b = b + 2.0;
    d = 1.0 / (a * d + b);
    c = b + a / c;
    const double delta = c * d;
    h = h * delta;
    if (fabs(delta - 1.0) <= step) break;
  }
  return h * exp(-x);
}

// sample m of the frame whose spectrum (Hermitian weights folded in) is Y [F + 1]:
// (sum_k re_k cos(2 pi k m / N) - sum_k im_k sin(2 pi k m / N)) / N, k ascending
__device__ __forceinline__ double dn_sample(const double2* Y, const double2* tw, int m, int F,
                                            int N) {
  double sc = 0.0, ss = 0.0;
  int idx = 0;
  for (int k = 0; k <= F; ++k) {
    const double2 w = tw[idx];
    const double2 v = Y[k];
    sc = fma(w.x, v.x, sc);
    ss = fma(w.y, v.y, ss);
    idx += m;
    if (idx >= N) idx -= N;
  }
  return (sc - ss) / (double)N;
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(192) void denoise_synthesis_kernel(
    const Tin* __restrict__ x, const int* __restrict__ lengths, int T, DnRate dr, int nfmax,
    const double2* __restrict__ twg, const double2* __restrict__ spec, Tout* __restrict__ y) {
  __shared__ double2 tw[2 * DN_MAX_F];
  __shared__ double2 Y[2][DN_MAX_F + 1];
  const int r = blockIdx.y, h = blockIdx.x, tid = threadIdx.x;
  const int F = dr.F, H = dr.H, N = dr.N;
  const int L = segan_row_samples(lengths, r, T);
  const int nf = dn_frames(L, dr);
  const long long n = (long long)h * H + tid;
  const bool inb = tid < H && n < T;
  if (nf == 0 || h > nf) {   // the whole workgroup, before any barrier
    if (inb) y[(size_t)r * T + n] = (nf == 0 && n < L) ? (Tout)x[(size_t)r * T + n] : (Tout)0;
    return;
  }
  // hop h <= nf: samples below (nf + 1) H <= L <= T; frame h - 1's second half, frame h's first
  const bool early = h >= 1, late = h < nf;
  dn_load_twiddles(tw, twg, N);
  for (int i = tid; i < 2 * (F + 1); i += blockDim.x) {
    const int which = i / (F + 1), k = i - which * (F + 1);
    if (which == 0 ? early : late) {
      const double2 v = spec[((size_t)r * nfmax + (h - 1 + which)) * (size_t)(F + 1) + k];
      const double ck = (k == 0 || k == F) ? 1.0 : 2.0;
      Y[which][k] = make_double2(ck * v.x, ck * v.y);
    }
  }
  __syncthreads();
  if (tid >= H) return;
  double o;
  if (early && late) {
    const double oa = dn_sample(Y[0], tw, tid + H, F, N);
    o = oa + dn_sample(Y[1], tw, tid, F, N);
  } else if (early) {
    o = dn_sample(Y[0], tw, tid + H, F, N);
  } else {
    o = dn_sample(Y[1], tw, tid, F, N);
  }
  y[(size_t)r * T + n] = (Tout)o;
}

bool dn_sizes_ok(int rows, int T) {
  return rows > 0 && rows <= 65535 && T > 0 && T <= DN_MAX_T;
}

}  // namespace
