// segan_whisper.hip — on-the-fly whispered speech: noise-excited LPC resynthesis (DESIGN.md section
// 18; the numpy oracle is scripts/whisper_oracle.py).  Per row: frames of 512 at a hop of 256 under
// a periodic Hann window, 17 lags, Levinson-Durbin of order 16, an all-pole filter per frame run
// over one continuous counter-based noise sequence, amplitude-complementary overlap-add, a peak
// guard.  All of it in fp64 with every operation rounded on its own; no atomics, no scratch; every
// sum runs in an order fixed by sample and frame index, so a row's result depends on neither the
// other rows nor T beyond its length.
#pragma clang fp contract(off)   // before the header: levinson_lpc rounds every operation here

#include "segan_signal.h"

#define WH_N SEGAN_WHISPER_N
#define WH_H SEGAN_WHISPER_H
#define WH_P SEGAN_WHISPER_P
#define WH_WU SEGAN_WHISPER_WU
#define WH_THREADS 256
#define WH_WAVES (WH_THREADS / 64)
#define WH_STEPS (WH_WU + WH_N)

static_assert(WH_N == 2 * WH_H && WH_N % 64 == 0, "two frames cover a sample; whole lanes");
static_assert(WH_WU % WH_P == 0 && WH_N % WH_P == 0, "the synthesis loop is unrolled by the order");

namespace {

// sqrt((2^64 - 1) / 3): the standard deviation of a sum of four uniform 32-bit words
constexpr double WH_C = 0x1.279a74590331cp+31;
constexpr double WH_WHITE = 1.0001;
constexpr double WH_EFLOOR = 0x1p-40;
constexpr double WH_WSUM2 = 192.0;   // sum of w^2 of the periodic Hann window of 512

__device__ __forceinline__ int wh_frames(int L) { return L / WH_H + 2; }

// Philox4x32-10 (Salmon et al., SC'11) of the counter (lo32(J), hi32(J), 0, 0) under the key
// (lo32(seed), hi32(seed)): u = (w0 + w1 + w2 + w3 - 2 (2^32 - 1)) / c, the sum in integers
__device__ __forceinline__ double wh_noise(unsigned long long J, unsigned k0, unsigned k1) {
  unsigned c0 = (unsigned)J, c1 = (unsigned)(J >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
  for (int rnd = 0; rnd < 10; ++rnd) {
    if (rnd) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
  }
  const long long s = (long long)((unsigned long long)c0 + c1 + c2 + c3) - 2ll * 0xFFFFFFFFll;
  return (double)s / WH_C;
}

__device__ __forceinline__ bool wh_tilt_ok(double tau) { return tau >= 0.0 && tau < 1.0; }

}  // namespace

// u [rows][count]: u[j0 + i] of each row's seed
__global__ __launch_bounds__(WH_THREADS) void whisper_noise_kernel(
    const long long* __restrict__ seeds, long long j0, int count, double* __restrict__ u) {
  const int r = blockIdx.y;
  const int i = blockIdx.x * WH_THREADS + threadIdx.x;
  if (i >= count) return;
  const unsigned long long seed = (unsigned long long)seeds[r];
  const unsigned long long J = (unsigned long long)(j0 + (long long)i + (1ll << 20));
  u[(size_t)r * count + i] = wh_noise(J, (unsigned)seed, (unsigned)(seed >> 32));
}

// ---------------------------------------------------------------------------------
// Lags.  One wave per (frame, row), four frames per workgroup.  s = w xe sits in LDS with WH_P
// zeros behind it; lane i sums s[m] s[m + l] over m = i, i + 64, .. ascending, the 64 partial sums
// meet in the xor butterfly (32, 16 .. 1).  r[l] <- r[l] g[l], then r[0] <- r[0] 1.0001.
// Frames from the row's own count up to Fmax see zeros only and come out zero.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(WH_THREADS) void whisper_lags_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const float* __restrict__ prev,
    const double* __restrict__ window, const double* __restrict__ lagwin, double* __restrict__ r,
    int T, int Fmax) {
  __shared__ double sh[WH_WAVES][WH_N + WH_P];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * WH_WAVES + wave, row = blockIdx.y;
  const int L = segan_row_samples(lengths, row, T);
  const float* xr = x + (size_t)row * T;
  const float pv = prev ? prev[row] : 0.0f;
  double* s = sh[wave];
  if (f < Fmax) {
    const long long jb = ((long long)f - 1) * WH_H;
    for (int m = lane; m < WH_N; m += 64) {
      const long long j = jb + m;
      const float v = j == 0 ? pv : (j > 0 && j <= L ? xr[j - 1] : 0.0f);
      s[m] = window[m] * (double)v;
    }
    if (lane < WH_P) s[WH_N + lane] = 0.0;
  }
  __syncthreads();
  if (f >= Fmax) return;

  double acc[WH_P + 1];
#pragma unroll
  for (int l = 0; l <= WH_P; ++l) acc[l] = 0.0;
  for (int m = lane; m < WH_N; m += 64) {
    const double a = s[m];
#pragma unroll
    for (int l = 0; l <= WH_P; ++l) {
      const double p = a * s[m + l];
      acc[l] = acc[l] + p;
    }
  }
  double mine = 0.0;   // lane l keeps lag l
#pragma unroll
  for (int l = 0; l <= WH_P; ++l) {
    const double t = segan_wave_sum(acc[l]);
    if (lane == l) mine = t;
  }
  if (lane <= WH_P) {
    mine = mine * lagwin[lane];
    if (lane == 0) mine = mine * WH_WHITE;
    r[((size_t)row * Fmax + f) * (WH_P + 1) + lane] = mine;
  }
}

// ---------------------------------------------------------------------------------
// LPC.  One thread per set of lags: Levinson-Durbin with its two guards (levinson_lpc),
// sigma = sqrt(E / 192), the order reached.  r[0] <= 0 (or NaN): a = [1, 0 ..], sigma = 0, order 0.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void whisper_lpc_kernel(const double* __restrict__ r, long long n,
                                                         double* __restrict__ a,
                                                         double* __restrict__ sigma,
                                                         int* __restrict__ order) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  double R[WH_P + 1], A[WH_P + 1];
#pragma unroll
  for (int l = 0; l <= WH_P; ++l) R[l] = r[i * (WH_P + 1) + l];
  double E = 0.0;
  int ord = 0;
  if (R[0] > 0.0) {
    levinson_lpc<WH_P, false, true>(R, A, WH_EFLOOR, &E, &ord);
  } else {
    A[0] = 1.0;
#pragma unroll
    for (int l = 1; l <= WH_P; ++l) A[l] = 0.0;
  }
#pragma unroll
  for (int l = 0; l <= WH_P; ++l) a[i * (WH_P + 1) + l] = A[l];
  sigma[i] = sqrt(E / WH_WSUM2);
  order[i] = ord;
}

// ---------------------------------------------------------------------------------
// Synthesis.  One lane per (frame, row): from zero state over j = (f-1) H - WU .. (f+1) H - 1,
//   e[j] = (sigma (u[j] - tau u[j-1])) / sqrt(1 + tau tau)
//   v[j] = e[j] - a[P] v[j-P] - .. - a[1] v[j-1]      (k descending: v[j-1] enters last)
// The last P outputs live in registers; the time loop is unrolled by P so that every index into
// them is a constant.  After the warm-up, w[m] v goes to ws[row][m][f]: the frame index runs
// fastest, so a wave's store is contiguous.  A silent frame stores zeros.  Lanes past the row's
// frames, and rows whose tilt is refused, store nothing: the overlap-add reads none of that.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void whisper_synth_kernel(
    const int* __restrict__ lengths, const double* __restrict__ r, const double* __restrict__ a,
    const double* __restrict__ sigma, const long long* __restrict__ seeds,
    const double* __restrict__ tilts, const double* __restrict__ window, double* __restrict__ ws,
    int T, int Fmax) {
  const int f = blockIdx.x * 64 + threadIdx.x, row = blockIdx.y;
  const int L = segan_row_samples(lengths, row, T);
  const double tau = tilts[row];
  if (f >= wh_frames(L) || !wh_tilt_ok(tau)) return;
  const size_t fi = (size_t)row * Fmax + f;
  const bool silent = !(r[fi * (WH_P + 1)] > 0.0);
  double A[WH_P + 1];
#pragma unroll
  for (int k = 0; k <= WH_P; ++k) A[k] = a[fi * (WH_P + 1) + k];
  const double sg = sigma[fi];
  const double den = sqrt(1.0 + tau * tau);
  const unsigned long long seed = (unsigned long long)seeds[row];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
  // counter of j = (f-1) H - WU; never negative: j >= -H - WU - 1 > -2^20
  unsigned long long J = (unsigned long long)(((long long)f - 1) * WH_H - WH_WU + (1ll << 20));
  double uprev = wh_noise(J - 1, k0, k1);
  double v[WH_P];
#pragma unroll
  for (int k = 0; k < WH_P; ++k) v[k] = 0.0;
  double* out = ws + (size_t)row * WH_N * Fmax + f;

  for (int blk = 0; blk < WH_STEPS / WH_P; ++blk) {
#pragma unroll
    for (int s = 0; s < WH_P; ++s) {
      const double u = wh_noise(J, k0, k1);
      ++J;
      const double tu = tau * uprev;
      const double d = u - tu;
      const double se = sg * d;
      double acc = se / den;
      uprev = u;
#pragma unroll
      for (int k = WH_P; k >= 1; --k) {
        const double p = A[k] * v[(s - k + 2 * WH_P) % WH_P];
        acc = acc - p;
      }
      v[s] = acc;
      const int m = blk * WH_P + s - WH_WU;
      if (m >= 0) {
        const double wv = window[m] * acc;
        out[(size_t)m * Fmax] = silent ? 0.0 : wv;
      }
    }
  }
}

// ---------------------------------------------------------------------------------
// Overlap-add, peak guard, output.  One workgroup per row.  y[j] = ws[q][j - q H + H] + ws[q + 1][j
// - q H], q = j / H (the earlier frame first), j = 0 .. len; m = max |y| (exact in any order); a
// second pass forms y again, divides by m when m > 1 and rounds once.  out[n] = y[n + 1], zero from
// len on; prev_out = y[0].  A row whose frames are all silent, or whose tilt is outside [0, 1),
// is copied with its prev.
// ---------------------------------------------------------------------------------
template <typename TY>
__global__ __launch_bounds__(WH_THREADS) void whisper_ola_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const float* __restrict__ prev,
    const double* __restrict__ r, const int* __restrict__ order, const double* __restrict__ tilts,
    const double* __restrict__ ws, TY* __restrict__ y, TY* __restrict__ prev_out,
    double* __restrict__ peak, int* __restrict__ status, int* __restrict__ nsilent,
    int* __restrict__ minorder, int T, int Fmax) {
  __shared__ int shn[WH_WAVES], sho[WH_WAVES];
  __shared__ double shm[WH_WAVES];
  const int row = blockIdx.x, t = threadIdx.x;
  const int L = segan_row_samples(lengths, row, T);
  const int F = wh_frames(L);
  const float* xr = x + (size_t)row * T;
  TY* yr = y + (size_t)row * T;
  const double* wr = ws + (size_t)row * WH_N * Fmax;

  int ns = 0, mo = WH_P;
  for (int f = t; f < F; f += WH_THREADS) {
    const size_t fi = (size_t)row * Fmax + f;
    if (r[fi * (WH_P + 1)] > 0.0)
      mo = min(mo, order[fi]);
    else
      ++ns;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ns += __shfl_xor(ns, o, 64);
    mo = min(mo, __shfl_xor(mo, o, 64));
  }
  if ((t & 63) == 0) {
    shn[t >> 6] = ns;
    sho[t >> 6] = mo;
  }
  __syncthreads();
  ns = 0;
  mo = WH_P;
#pragma unroll
  for (int w = 0; w < WH_WAVES; ++w) {
    ns += shn[w];
    mo = min(mo, sho[w]);
  }
  const int st = (wh_tilt_ok(tilts[row]) ? 0 : SEGAN_WHISPER_ST_TILT) |
                 (ns == F ? SEGAN_WHISPER_ST_SILENT : 0);
  if (t == 0) {
    status[row] = st;
    nsilent[row] = ns;
    minorder[row] = mo;
  }
  if (st) {   // uniform over the workgroup
    for (int i = t; i < T; i += WH_THREADS) yr[i] = (TY)xr[i];
    if (t == 0) {
      prev_out[row] = (TY)(prev ? prev[row] : 0.0f);
      peak[row] = 0.0;
    }
    return;
  }

  double m = 0.0;
  for (int j = t; j <= L; j += WH_THREADS) {
    const int q = j / WH_H, p = j - q * WH_H;
    const double v = wr[(size_t)(p + WH_H) * Fmax + q] + wr[(size_t)p * Fmax + q + 1];
    m = fmax(m, fabs(v));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) shm[t >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < WH_WAVES; ++w) m = fmax(m, shm[w]);
  const bool guard = m > 1.0;

  for (int j = t; j <= T; j += WH_THREADS) {
    double v = 0.0;
    if (j <= L) {
      const int q = j / WH_H, p = j - q * WH_H;
      v = wr[(size_t)(p + WH_H) * Fmax + q] + wr[(size_t)p * Fmax + q + 1];
      if (guard) v = v / m;
    }
    if (j == 0)
      prev_out[row] = (TY)v;
    else
      yr[j - 1] = (TY)v;
  }
  if (t == 0) peak[row] = m;
}

static int wh_rows_ok(const char* what, int rows, int T) {
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && T > 0 && (long long)T <= (1ll << 30),
                "%s: bad sizes rows=%d T=%d", what, rows, T);
  return SEGAN_OK;
}

extern "C" int segan_whisper_frames(int T) { return T < 0 ? 0 : T / WH_H + 2; }

// doubles: r and a [rows][F][P + 1], sigma [rows][F], the windowed outputs [rows][N][F], then
// order int[rows][F] in the doubles that follow
extern "C" long long segan_whisper_ws_doubles(int rows, int T) {
  if (rows <= 0 || T <= 0) return 0;
  const long long nf = (long long)rows * segan_whisper_frames(T);
  return nf * (2 * (WH_P + 1) + 1 + WH_N) + (nf + 1) / 2;
}

extern "C" int segan_whisper_noise(const long long* seeds, long long j0, int count, int rows,
                                   double* u, void* stream) {
  SEGAN_REQUIRE(seeds && u, "whisper_noise: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && count > 0, "whisper_noise: bad sizes rows=%d count=%d",
                rows, count);
  SEGAN_REQUIRE(j0 >= -(1ll << 20) && j0 <= (1ll << 31),
                "whisper_noise: j0 = %lld outside -2^20 .. 2^31", j0);
  hipLaunchKernelGGL(whisper_noise_kernel, dim3(ceil_div(count, WH_THREADS), rows),
                     dim3(WH_THREADS), 0, (hipStream_t)stream, seeds, j0, count, u);
  return segan_check_launch("whisper_noise_kernel");
}

extern "C" int segan_whisper_lags(const float* x, const int* lengths, const float* prev,
                                  const double* window, const double* lagwin, int rows, int T,
                                  double* r, void* stream) {
  SEGAN_REQUIRE(x && window && lagwin && r, "whisper_lags: NULL pointer");
  if (int e = wh_rows_ok("whisper_lags", rows, T)) return e;
  const int Fmax = segan_whisper_frames(T);
  hipLaunchKernelGGL(whisper_lags_kernel, dim3(ceil_div(Fmax, WH_WAVES), rows), dim3(WH_THREADS),
                     0, (hipStream_t)stream, x, lengths, prev, window, lagwin, r, T, Fmax);
  return segan_check_launch("whisper_lags_kernel");
}

extern "C" int segan_whisper_lpc(const double* r, long long n, double* a, double* sigma,
                                 int* order, void* stream) {
  SEGAN_REQUIRE(r && a && sigma && order, "whisper_lpc: NULL pointer");
  SEGAN_REQUIRE(n > 0 && n <= (1ll << 31) - 64, "whisper_lpc: bad count %lld", n);
  hipLaunchKernelGGL(whisper_lpc_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, r, n, a, sigma, order);
  return segan_check_launch("whisper_lpc_kernel");
}

extern "C" int segan_whisper_synth(const float* x, const int* lengths, const float* prev,
                                   const double* r, const double* a, const double* sigma,
                                   const int* order, const long long* seeds, const double* tilts,
                                   const double* window, int rows, int T, double* ws,
                                   long long ws_doubles, void* y, int y_dtype, void* prev_out,
                                   double* peak, int* status, int* nsilent, int* minorder,
                                   void* stream) {
  SEGAN_REQUIRE(x && r && a && sigma && order && seeds && tilts && window && ws && y && prev_out &&
                    peak && status && nsilent && minorder,
                "whisper_synth: NULL pointer");
  if (int e = wh_rows_ok("whisper_synth", rows, T)) return e;
  SEGAN_REQUIRE(y_dtype == SEGAN_DT_F32 || y_dtype == SEGAN_DT_F64,
                "whisper_synth: y_dtype %d is neither fp32 nor fp64", y_dtype);
  const int Fmax = segan_whisper_frames(T);
  SEGAN_REQUIRE(ws_doubles >= (long long)rows * WH_N * Fmax,
                "whisper_synth: workspace of %lld doubles, %lld needed", ws_doubles,
                (long long)rows * WH_N * Fmax);
  hipLaunchKernelGGL(whisper_synth_kernel, dim3(ceil_div(Fmax, 64), rows), dim3(64), 0,
                     (hipStream_t)stream, lengths, r, a, sigma, seeds, tilts, window, ws, T, Fmax);
  if (int e = segan_check_launch("whisper_synth_kernel")) return e;
  if (y_dtype == SEGAN_DT_F64)
    hipLaunchKernelGGL(whisper_ola_kernel<double>, dim3(rows), dim3(WH_THREADS), 0,
                       (hipStream_t)stream, x, lengths, prev, r, order, tilts, ws, (double*)y,
                       (double*)prev_out, peak, status, nsilent, minorder, T, Fmax);
  else
    hipLaunchKernelGGL(whisper_ola_kernel<float>, dim3(rows), dim3(WH_THREADS), 0,
                       (hipStream_t)stream, x, lengths, prev, r, order, tilts, ws, (float*)y,
                       (float*)prev_out, peak, status, nsilent, minorder, T, Fmax);
  return segan_check_launch("whisper_ola_kernel");
}

extern "C" int segan_whisper_rows(const float* x, const int* lengths, const float* prev,
                                  const long long* seeds, const double* tilts,
                                  const double* window, const double* lagwin, int rows, int T,
                                  double* ws, long long ws_doubles, void* y, int y_dtype,
                                  void* prev_out, double* peak, int* status, int* nsilent,
                                  int* minorder, void* stream) {
  SEGAN_REQUIRE(ws, "whisper_rows: NULL pointer");
  if (int e = wh_rows_ok("whisper_rows", rows, T)) return e;
  SEGAN_REQUIRE(ws_doubles >= segan_whisper_ws_doubles(rows, T),
                "whisper_rows: workspace of %lld doubles, %lld needed", ws_doubles,
                segan_whisper_ws_doubles(rows, T));
  const long long nf = (long long)rows * segan_whisper_frames(T);
  double* r = ws;
  double* a = r + nf * (WH_P + 1);
  double* sigma = a + nf * (WH_P + 1);
  double* wv = sigma + nf;
  int* order = (int*)(wv + nf * WH_N);
  if (int e = segan_whisper_lags(x, lengths, prev, window, lagwin, rows, T, r, stream)) return e;
  if (int e = segan_whisper_lpc(r, nf, a, sigma, order, stream)) return e;
  return segan_whisper_synth(x, lengths, prev, r, a, sigma, order, seeds, tilts, window, rows, T,
                             wv, nf * WH_N, y, y_dtype, prev_out, peak, status, nsilent, minorder,
                             stream);
}
