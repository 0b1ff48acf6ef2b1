// What the fp64 signal files (audio, quality, BSS-eval, STOI, additive, resample) share: each piece here has
// more than one user.  The Hann windows are NOT here: quality, STOI and SSNR each round theirs
// the way their own oracle does.
#pragma once
#include "segan_common.h"
#include <math.h>
#include <deque>
#include <mutex>
#include <vector>

// fp64 sum over the wave by a fixed xor butterfly; the result is in every lane
__device__ __forceinline__ double segan_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sums of N values over a 256-thread workgroup in a fixed order (butterfly, then the four
// waves in turn); the result is in every thread
template <int N>
__device__ __forceinline__ void block_sum_fixed(double (&v)[N], double (*sh)[N]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    v[j] = segan_wave_sum(v[j]);
    if (lane == 0) sh[wave][j] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
}

// the row's valid samples: lengths[r] clamped to [0, T] (all T without lengths)
__device__ __forceinline__ int segan_row_samples(const int* __restrict__ lengths, int r, int T) {
  if (!lengths) return T;
  const int L = lengths[r];
  return L < 0 ? 0 : (L > T ? T : L);
}

// Levinson-Durbin in fp64 (lpcoeff, utils.py:659-716), every lane on its own: A = [1, -a] of the
// order-P predictor of the lags R.  ROUND32: A rounded to fp32 as lpcoeff returns it (LLR).
// GUARD (the whisper stage): the recursion stops at order m - 1, with the higher coefficients
// zero, when the reflection coefficient k_m is not |k_m| < 1 or when the error E has fallen to
// efloor R[0]; *Eout and *order are then what that order left.  Without GUARD the operations and
// their order are what LLR and CD have always run; Eout and order are not touched.
template <int P, bool ROUND32 = true, bool GUARD = false>
__device__ __forceinline__ void levinson_lpc(const double (&R)[P + 1], double (&A)[P + 1],
                                             double efloor = 0.0, double* Eout = nullptr,
                                             int* order = nullptr) {
  double a[P];
#pragma unroll
  for (int j = 0; j < P; ++j) a[j] = 1.0;
  double E = R[0];
  const double floorE = efloor * R[0];
  bool go = true;
  int ord = 0;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    if (GUARD) go = go && E > floorE;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j) sum += a[j] * R[i - j];
    const double rc = (R[i + 1] - sum) / E;
    if (GUARD) go = go && fabs(rc) < 1.0;
    if (!GUARD || go) {
      double na[P];
#pragma unroll
      for (int j = 0; j < i; ++j) na[j] = a[j] - rc * a[i - 1 - j];
#pragma unroll
      for (int j = 0; j < i; ++j) a[j] = na[j];
      a[i] = rc;
      E = (1 - rc * rc) * E;
      ord = i + 1;
    }
  }
  A[0] = 1.0;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const double c = (GUARD && j >= ord) ? 0.0 : -a[j];
    A[j + 1] = ROUND32 ? (double)(float)c : c;
  }
  if (GUARD) {
    *Eout = E;
    *order = ord;
  }
}

// ceil(L p / q): the samples L samples become when resampled by p / q
__host__ __device__ inline long long segan_resampled_len(long long L, int p, int q) {
  return (L * p + q - 1) / q;
}

// (cos, sin)(2 pi m / n), m = 0 .. n - 1
inline std::vector<double2> segan_twiddles(int n) {
  std::vector<double2> tw(n);
  for (int m = 0; m < n; ++m) {
    const double ang = 2.0 * M_PI * (double)m / (double)n;
    tw[m] = make_double2(cos(ang), sin(ang));
  }
  return tw;
}

// Host-built tables that live on a device.  E has an `int device`; get() returns the entry of the
// current device that `match` accepts, or has `build` fill a new one (device already set; false
// with the error set on failure) under the lock.  Entries are never freed or moved.
template <typename E>
struct SeganDeviceTables {
  std::mutex mu;
  std::deque<E> entries;   // push_back keeps earlier elements in place

  template <typename Match, typename Build>
  const E* get(const char* what, Match match, Build build) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
      segan_set_error("%s: hipGetDevice failed", what);
      return nullptr;
    }
    std::lock_guard<std::mutex> lock(mu);
    for (const E& e : entries)
      if (e.device == dev && match(e)) return &e;
    E e{};
    e.device = dev;
    if (!build(&e)) return nullptr;
    entries.push_back(e);
    return &entries.back();
  }
};

template <typename V>
bool segan_upload(V** dst, const std::vector<V>& src, const char* what) {
  const size_t bytes = src.size() * sizeof(V);
  if (hipMalloc(dst, bytes) == hipSuccess &&
      hipMemcpy(*dst, src.data(), bytes, hipMemcpyHostToDevice) == hipSuccess)
    return true;
  segan_set_error("%s: table upload failed", what);
  return false;
}

// ---- the framing of the pitch trackers (segan_pitch.hip, segan_pyin.hip) ----

#define PITCH_MAX_H 80         // the 16 kHz constants; 8 kHz halves them
#define PITCH_MAX_LAGS 268     // lags 0 .. tau_max + 1
#define PITCH_MAX_T (1 << 24)

struct PitchRate {
  int H, tmin, tmax, nl;   // hop, smallest and largest lag, lags computed (tau_max + 2)
};

__host__ __device__ inline bool pitch_rate(int srate, PitchRate* p) {
  if (srate != 16000 && srate != 8000) return false;
  const int div = srate == 16000 ? 1 : 2;
  p->H = PITCH_MAX_H / div;
  p->tmin = 40 / div;
  p->tmax = 266 / div;
  p->nl = p->tmax + 2;
  return true;
}

// hop blocks of a row of L samples: every index j + tau of a block stays below L
__host__ __device__ inline int pitch_blocks(int L, int H, int nl) {
  return L >= nl - 1 ? (L - (nl - 1)) / H : 0;
}

__host__ __device__ inline int pitch_frames_of(int nb) {
  return nb >= SEGAN_PITCH_NB ? nb - SEGAN_PITCH_NB + 1 : 0;
}

inline bool segan_pitch_sizes_ok(int rows, int T) {
  return rows > 0 && rows <= 65535 && T > 0 && T <= PITCH_MAX_T;
}

// ---- defined in segan_pitch.hip ----

// segan_pitch_cmnd with c(tau_max + 1) of every frame of a row's own count as well: cmnd
// [rows][F][nl], ctot [rows][F] (frames past a row's count are not written), ws as segan_pitch's.
// The arguments are the caller's to check.
int segan_pitch_cmnd_ctot(const float* x, const int* lengths, int rows, int T, int srate,
                          double* cmnd, double* ctot, double* ws, hipStream_t stream);

// ---- defined in segan_resample.hip ----

// p / q = num / den in lowest terms
void segan_reduce_ratio(int num, int den, int* p, int* q);

// The 2 zeros max(p, q) + 1 taps p h / sum(h) of the Kaiser-windowed sinc h (p == q == 1: [1.0]).
// compensate = false normalises by the index-order sum of h, always; true swaps in a compensated
// sum where the index order alone would move the largest tap by more than 1e-15.
void segan_kaiser_sinc_taps(int p, int q, int zeros, double beta, bool compensate,
                            std::vector<double>* taps);

// The polyphase resampling of rows x [rows][T] (SEGAN_DT_F32 / I16) by p / q into y
// [rows][Ly_max] (SEGAN_DT_F64 / F32 / I16): table lookup and launch.  The limits are the
// callers': segan_resample applies the public ones, segan_stoi takes every rate from 4 to 48 kHz
// (up to p / q = 10000 / 47999).  The kernel indexes its tap table with int, below
// 2 zeros max(p, q) + p: under 1e6 for either caller.  out_lengths, tile_clip: optional (see
// resample_kernel).  SEGAN_OK, or SEGAN_ELAUNCH when the table cannot be built.
int segan_resample_rows(int p, int q, int zeros, double beta, bool compensate, const void* x,
                        int x_dtype, const int* lengths, int rows, int T, void* y, int y_dtype,
                        int Ly_max, int* out_lengths, int* tile_clip, hipStream_t stream);
