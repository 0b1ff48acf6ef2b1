// The radix-2 Stockham transform on complex doubles in LDS that segan_srmr.hip (fft_kernel) and
// segan_dereverb.hip (the STFT of WPE) share: the passes, the twiddle table and the complex
// product with its roundings spelled out.  A workgroup of FFT_THREADS threads transforms one
// sequence of up to FFT_LDS_N values, or 2^lgbatch interleaved ones.
#pragma once
#include "segan_signal.h"

#define FFT_THREADS 256
#define FFT_LDS_LOG2 SEGAN_FFT_LDS_LOG2
#define FFT_LDS_N (1 << FFT_LDS_LOG2)
#define FFT_BFLY (FFT_LDS_N / 2 / FFT_THREADS)   // butterflies a thread holds in registers

static_assert(FFT_BFLY * 2 * FFT_THREADS == FFT_LDS_N, "fft: whole butterflies per thread");

namespace {

// (x + i y)(c + i s) with its roundings spelled out: the bits do not hang on what the compiler
// chooses to contract
__device__ __forceinline__ double2 cmul(double x, double y, double c, double s) {
  return make_double2(fma(x, c, -(y * s)), fma(x, s, y * c));
}

// The lgsub passes over sm, which holds 2^lgbatch interleaved sequences of 2^lgsub values:
// element i of sequence t at sm[(i << lgbatch) | t] going in, output k of sequence t at
// sm[(k << lgbatch) | t] coming out.  tw = (cos, sin)(2 pi m / FFT_LDS_N), m < FFT_LDS_N / 2.
// Every thread of the workgroup calls it, after a barrier behind the writes of sm; it ends behind
// a barrier.  Stockham: pass p pairs x[j], x[j + M/2] and writes them 2^p transforms' stride
// apart; the interleaved transforms ride along as the low bits of j.
__device__ __forceinline__ void fft_lds_passes(double2* sm, const double2* __restrict__ tw,
                                               int lgsub, int lgbatch, bool inverse) {
  const int tid = threadIdx.x;
  const int half = (1 << (lgsub + lgbatch)) >> 1;
  for (int pass = 0; pass < lgsub; ++pass) {
    const int lgs = lgbatch + pass;
    double2 y0[FFT_BFLY], y1[FFT_BFLY];
#pragma unroll
    for (int u = 0; u < FFT_BFLY; ++u) {
      const int j = tid + FFT_THREADS * u;
      if (j < half) {
        const double2 p0 = sm[j], p1 = sm[j + half];
        const int p = j >> lgs;
        const double2 w = tw[p << (pass + FFT_LDS_LOG2 - lgsub)];
        const double ws = inverse ? w.y : -w.y;
        const double dx = p0.x - p1.x, dy = p0.y - p1.y;
        y0[u] = make_double2(p0.x + p1.x, p0.y + p1.y);
        y1[u] = cmul(dx, dy, w.x, ws);
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < FFT_BFLY; ++u) {
      const int j = tid + FFT_THREADS * u;
      if (j < half) {
        const int p = j >> lgs, q = j & ((1 << lgs) - 1);
        sm[q + ((2 * p) << lgs)] = y0[u];
        sm[q + ((2 * p + 1) << lgs)] = y1[u];
      }
    }
    __syncthreads();
  }
}

// ---- the twiddle table, one per device ----

struct FftTable {
  int device;
  double2* tw;
};
SeganDeviceTables<FftTable> g_fft_tables;

const FftTable* fft_table() {
  return g_fft_tables.get(
      "fft", [](const FftTable&) { return true; },
      [](FftTable* e) {
        std::vector<double2> tw(FFT_LDS_N / 2);
        for (int m = 0; m < FFT_LDS_N / 2; ++m) {   // rounded from extended precision
          const long double ang = 2.0L * 3.14159265358979323846264338327950288L * m / FFT_LDS_N;
          tw[m] = make_double2((double)cosl(ang), (double)sinl(ang));
        }
        tw[FFT_LDS_N / 4] = make_double2(0.0, 1.0);
        return segan_upload(&e->tw, tw, "fft");
      });
}

}  // namespace
