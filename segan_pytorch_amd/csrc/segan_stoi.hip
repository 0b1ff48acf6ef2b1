// segan_stoi.hip — STOI, Taal et al.'s short-time objective intelligibility, of rows of clean /
// processed signals, fp64 throughout (DESIGN.md section 10 states the rules; the numpy oracle is
// scripts/stoi_oracle.py).  Seven stages, each one launch for all rows (stage 1: one per signal),
// the per-row counts (resampled length, frames, kept frames) derived on the device from `lengths`
// and `count`:
//   resample to 10 kHz -> frame energies -> keep mask, kept-frame list, M -> overlap-add
//   compaction -> third-octave band envelopes -> segment correlations -> per-row mean.
// Stage 1 is the library's one resampling kernel (segan_resample_rows, segan_resample.hip) with
// fp64 output, and the taps are the one designer's (segan_kaiser_sinc_taps) at (zeros, beta) =
// (10, 5.0) in its index-order mode: STOI's taps are pinned to its oracle at every integer rate
// from 4 to 48 kHz, the public converter's compensated normalisation differs from them at some
// (11025 and 37800 Hz among them).  Window, twiddles and the band table are built on the host
// once per (device, srate).
// Every sum runs in a fixed order that depends only on the row's own data: a row's result does
// not depend on the other rows, on T or on the launch.
// ESTOI (Jensen & Taal 2016; segan_estoi, oracle scripts/estoi_oracle.py) shares stages 1-5
// (stoi_front) and replaces the last two: each 15 x 30 window of X and of Y is normalised along
// its rows and then along its columns, d_s is their inner product / 30, d the mean of d_s.
#include "segan_signal.h"

#define ST_FS 10000       // internal rate
#define ST_N 256          // frame
#define ST_K 128          // hop
#define ST_NFFT 512
#define ST_J 15           // third-octave bands
#define ST_SEG 30         // band frames per segment
#define ST_SRATE_MIN 4000
#define ST_SRATE_MAX 48000
#define ST_THREADS 256

namespace {

struct BandTable {
  int lo[ST_J], hi[ST_J];   // DFT bins [lo, hi) of each band
};

bool srate_ok(int srate) { return srate >= ST_SRATE_MIN && srate <= ST_SRATE_MAX; }

// The resampling srate -> 10 kHz: p / q = 10000 / srate in lowest terms, the filter of
// scipy.signal.resample_poly's default (ST_ZEROS, ST_BETA), sum(h) in index order.
#define ST_ZEROS 10
#define ST_BETA 5.0

// Band i: the nearest bins (first of equals) to 150 * 2^((2i -+ 1)/6) Hz on k * 10000 / 512.
void make_bands(BandTable* bt) {
  for (int i = 0; i < ST_J; ++i) {
    const double f[2] = {150.0 * pow(2.0, (2 * i - 1) / 6.0), 150.0 * pow(2.0, (2 * i + 1) / 6.0)};
    int* dst[2] = {&bt->lo[i], &bt->hi[i]};
    for (int e = 0; e < 2; ++e) {
      int best = 0;
      double bd = INFINITY;
      for (int k = 0; k <= ST_NFFT / 2; ++k) {
        const double d = (double)k * ST_FS / ST_NFFT - f[e];
        if (d * d < bd) {
          bd = d * d;
          best = k;
        }
      }
      *dst[e] = best;
    }
  }
}

struct StoiTables {
  int device, srate, p, q, klo, nb;
  BandTable bands;
  double* window;   // [ST_N]
  double2* tw;      // [ST_NFFT]: (cos, sin)(2*pi*m/512)
};

SeganDeviceTables<StoiTables> g_tables;

const StoiTables* get_tables(int srate) {
  return g_tables.get(
      "stoi", [=](const StoiTables& t) { return t.srate == srate; },
      [=](StoiTables* t) {
        t->srate = srate;
        segan_reduce_ratio(ST_FS, srate, &t->p, &t->q);
        make_bands(&t->bands);
        t->klo = ST_NFFT;
        int khi = 0;
        for (int i = 0; i < ST_J; ++i) {
          t->klo = t->bands.lo[i] < t->klo ? t->bands.lo[i] : t->klo;
          khi = t->bands.hi[i] > khi ? t->bands.hi[i] : khi;
        }
        t->nb = khi - t->klo;
        std::vector<double> window(ST_N);
        for (int n = 0; n < ST_N; ++n)
          window[n] = 0.5 * (1.0 - cos(2.0 * M_PI * (n + 1) / (ST_N + 1)));
        return segan_upload(&t->window, window, "stoi") &&
               segan_upload(&t->tw, segan_twiddles(ST_NFFT), "stoi");
      });
}

struct StoiDims {
  int Ly, F, Lc, Fb, S;
};

// frames of ST_N at hop ST_K starting at 0, the last start at most L - N - 1
__host__ __device__ inline int stoi_frames(int L) { return L > ST_N ? (L - ST_N - 1) / ST_K + 1 : 0; }

// upper bounds of every stage's size for rows of at most T samples
int stoi_dims(const char* what, int T, int srate, StoiDims* d) {
  SEGAN_REQUIRE(srate_ok(srate), "%s: srate %d outside %d .. %d Hz", what, srate, ST_SRATE_MIN,
                ST_SRATE_MAX);
  SEGAN_REQUIRE(T >= 0, "%s: bad length T=%d", what, T);
  int p, q;
  segan_reduce_ratio(ST_FS, srate, &p, &q);
  const long long Ly = segan_resampled_len(T, p, q);
  SEGAN_REQUIRE(Ly <= (1ll << 30), "%s: T=%d resamples to %lld samples (at most 2^30)", what, T,
                Ly);
  d->Ly = (int)Ly;
  d->F = stoi_frames(d->Ly);
  d->Lc = d->F > 0 ? (d->F - 1) * ST_K + ST_N : 0;
  d->Fb = d->F > 1 ? d->F - 1 : 0;
  d->S = d->Fb >= ST_SEG ? d->Fb - ST_SEG + 1 : 0;
  return SEGAN_OK;
}

}  // namespace

__device__ __forceinline__ int row_resampled(const int* __restrict__ lengths, int r, int T, int p,
                                             int q) {
  return (int)segan_resampled_len(segan_row_samples(lengths, r, T), p, q);
}

// kept frames M -> band frames F' (the last kept frame never starts a band frame) -> segments
__device__ __forceinline__ int band_frames(int M) { return M > 1 ? M - 1 : 0; }
__device__ __forceinline__ int segments(int M) {
  const int Fb = band_frames(M);
  return Fb >= ST_SEG ? Fb - ST_SEG + 1 : 0;
}

// 1. Resample to 10 kHz: segan_resample_rows, once per signal.  Samples from the row's
// ceil(Lx p / q) up to Ly_max are zero.

// ---------------------------------------------------------------------------------
// 2. Frame energies of the clean signal, one wave per frame: 20 log10(||x_j w|| / sqrt(N)) dB,
// -inf for a frame of zeros.  Frames past the row's own count are NaN (never read).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_energy_kernel(
    const double* __restrict__ xr, const int* __restrict__ lengths, double* __restrict__ energy,
    int T, int Ly_max, int F_max, int p, int q, const double* __restrict__ window) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * (ST_THREADS / 64) + wave;
  const int r = blockIdx.y;
  if (j >= F_max) return;   // whole waves leave
  const int F = stoi_frames(row_resampled(lengths, r, T, p, q));
  double e = NAN;
  if (j < F) {
    const double* x = xr + (size_t)r * Ly_max + (size_t)j * ST_K;
    double s = 0.0;
#pragma unroll
    for (int n = lane; n < ST_N; n += 64) {
      const double v = x[n] * window[n];
      s = fma(v, v, s);
    }
    s = segan_wave_sum(s);
    e = 20.0 * log10(sqrt(s) / 16.0);   // sqrt(N) = 16
  }
  if (lane == 0) energy[(size_t)r * F_max + j] = e;
}

// ---------------------------------------------------------------------------------
// 3. One workgroup per row: the loudest frame, keep = E - max + 40 > 0 (a row of -inf keeps
// nothing: -inf - -inf is NaN), the keep mask, the ascending list of kept frames (ballot +
// popcount exclusive scan in chunks of 256) and their count M.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_select_kernel(
    const double* __restrict__ energy, const int* __restrict__ lengths, int* __restrict__ mask,
    int* __restrict__ kept, int* __restrict__ count, int T, int F_max, int p, int q) {
  __shared__ double wmax[ST_THREADS / 64];
  __shared__ int wcnt[ST_THREADS / 64];
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int F = stoi_frames(row_resampled(lengths, r, T, p, q));
  const double* E = energy + (size_t)r * F_max;
  double mx = -INFINITY;
  for (int j = t; j < F; j += ST_THREADS) mx = fmax(mx, E[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) wmax[wave] = mx;
  __syncthreads();
  mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));

  int* mrow = mask + (size_t)r * F_max;
  int* krow = kept + (size_t)r * F_max;
  int base = 0;
  for (int j0 = 0; j0 < F; j0 += ST_THREADS) {
    const int j = j0 + t;
    const bool keep = j < F && (E[j] - mx) + 40.0 > 0.0;
    const unsigned long long b = __ballot(keep);
    __syncthreads();   // wcnt of the previous chunk has been read
    if (lane == 0) wcnt[wave] = __popcll(b);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wcnt[w];
    if (j < F) mrow[j] = keep ? 1 : 0;
    if (keep) krow[off + __popcll(b & ((1ull << lane) - 1ull))] = j;
    base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
  }
  for (int j = F + t; j < F_max; j += ST_THREADS) mrow[j] = 0;
  if (t == 0) count[r] = base;
}

// ---------------------------------------------------------------------------------
// 4. Overlap-add compaction, one thread per output sample t of row blockIdx.y, signal
// blockIdx.z: the kept frames c = t/K - 1 and t/K (those that exist) windowed, earlier frame
// first.  Two terms (or one) per sample: the same sum as accumulating the frames in order.
// Compacted length (M - 1) K + N; zeros from there to Lc_max.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_compact_kernel(
    const double* __restrict__ xr, const double* __restrict__ yr, const int* __restrict__ kept,
    const int* __restrict__ count, double* __restrict__ xs, double* __restrict__ ys, int Ly_max,
    int F_max, int Lc_max, const double* __restrict__ window) {
  const int r = blockIdx.y;
  const int t = blockIdx.x * ST_THREADS + threadIdx.x;
  if (t >= Lc_max) return;
  const double* x = (blockIdx.z ? yr : xr) + (size_t)r * Ly_max;
  double* out = (blockIdx.z ? ys : xs) + (size_t)r * Lc_max;
  const int M = count[r];
  const int Lc = M > 0 ? (M - 1) * ST_K + ST_N : 0;
  double v = 0.0;
  if (t < Lc) {
    const int* krow = kept + (size_t)r * F_max;
    const int c1 = t / ST_K, n1 = t - c1 * ST_K;   // c1 <= M
    const double a1 = c1 < M ? x[(size_t)krow[c1] * ST_K + n1] * window[n1] : 0.0;
    if (c1 > 0) {
      const int n0 = n1 + ST_K;
      const double a0 = x[(size_t)krow[c1 - 1] * ST_K + n0] * window[n0];
      v = c1 < M ? a0 + a1 : a0;
    } else {
      v = a1;
    }
  }
  out[t] = v;
}

// ---------------------------------------------------------------------------------
// 5. Band envelopes, one 256-thread workgroup per (band frame f, row): both compacted frames
// windowed again into LDS with the twiddles, |X_k|^2 of the 512-point DFT (zero padding adds
// nothing) as a direct fp64 sum over the bins [klo, klo + nb) the bands cover, one thread per
// bin; then one thread per (band, signal) sums its bins in ascending order, sqrt.
// X, Y: [rows][15][Fb_max].
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_band_kernel(
    const double* __restrict__ xs, const double* __restrict__ ys, const int* __restrict__ count,
    double* __restrict__ X, double* __restrict__ Y, int Lc_max, int Fb_max, int klo, int nb,
    BandTable bt, const double* __restrict__ window, const double2* __restrict__ twg) {
  __shared__ double2 fr[ST_N];
  __shared__ double2 tw[ST_NFFT];
  __shared__ double2 spec[ST_NFFT / 2 + 1];
  const int f = blockIdx.x, r = blockIdx.y, t = threadIdx.x;
  if (f >= band_frames(count[r])) return;   // whole workgroup leaves
  const size_t base = (size_t)r * Lc_max + (size_t)f * ST_K;
  for (int n = t; n < ST_N; n += ST_THREADS) {
    const double w = window[n];
    fr[n] = make_double2(xs[base + n] * w, ys[base + n] * w);
  }
  for (int m = t; m < ST_NFFT; m += ST_THREADS) tw[m] = twg[m];
  __syncthreads();

  for (int b = t; b < nb; b += ST_THREADS) {
    const int k = klo + b;
    double xr = 0.0, xi = 0.0, yr = 0.0, yi = 0.0;
    int idx = 0;
    for (int n = 0; n < ST_N; ++n) {
      const double2 v = fr[n];
      const double2 w = tw[idx];
      xr = fma(v.x, w.x, xr);
      xi = fma(v.x, w.y, xi);
      yr = fma(v.y, w.x, yr);
      yi = fma(v.y, w.y, yi);
      idx = (idx + k) & (ST_NFFT - 1);
    }
    spec[b] = make_double2(xr * xr + xi * xi, yr * yr + yi * yi);
  }
  __syncthreads();
  if (t < 2 * ST_J) {
    const int i = t % ST_J, sig = t / ST_J;
    double e = 0.0;
    for (int k = bt.lo[i]; k < bt.hi[i]; ++k) e += sig ? spec[k - klo].y : spec[k - klo].x;
    (sig ? Y : X)[((size_t)r * ST_J + i) * Fb_max + f] = sqrt(e);
  }
}

// ---------------------------------------------------------------------------------
// 6. Segment correlations, one thread per (segment s, band i) of row blockIdx.y: the band
// frames m - 29 .. m, m = 29 + s, of X and Y; alpha = sqrt(sum X^2 / sum Y^2); Y' =
// fmin(alpha Y, X + X*clip) — fmin returns the other operand of a NaN, so an all-zero Y window
// (alpha = inf, 0 * inf = NaN) gives Y' = X + X*clip; the Pearson correlation of X and Y' (0/0
// is NaN).  rho: [rows][S_max][15].
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_segment_kernel(
    const double* __restrict__ X, const double* __restrict__ Y, const int* __restrict__ count,
    double* __restrict__ rho, int Fb_max, int S_max, double clip) {
  const int r = blockIdx.y;
  const int g = blockIdx.x * ST_THREADS + threadIdx.x;
  if (g >= S_max * ST_J) return;
  const int s = g / ST_J, i = g - s * ST_J;
  if (s >= segments(count[r])) return;
  const double* xrow = X + ((size_t)r * ST_J + i) * Fb_max + s;
  const double* yrow = Y + ((size_t)r * ST_J + i) * Fb_max + s;
  double x[ST_SEG], y[ST_SEG];
  double sxx = 0.0, syy = 0.0;
#pragma unroll
  for (int k = 0; k < ST_SEG; ++k) {
    x[k] = xrow[k];
    y[k] = yrow[k];
    sxx = fma(x[k], x[k], sxx);
    syy = fma(y[k], y[k], syy);
  }
  const double alpha = sqrt(sxx / syy);
  double mx = 0.0, my = 0.0;
#pragma unroll
  for (int k = 0; k < ST_SEG; ++k) {
    y[k] = fmin(alpha * y[k], x[k] + x[k] * clip);
    mx += x[k];
    my += y[k];
  }
  mx /= ST_SEG;
  my /= ST_SEG;
  double nx = 0.0, ny = 0.0;
#pragma unroll
  for (int k = 0; k < ST_SEG; ++k) {
    x[k] -= mx;
    y[k] -= my;
    nx = fma(x[k], x[k], nx);
    ny = fma(y[k], y[k], ny);
  }
  nx = sqrt(nx);
  ny = sqrt(ny);
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < ST_SEG; ++k) acc = fma(x[k] / nx, y[k] / ny, acc);
  rho[((size_t)r * S_max + s) * ST_J + i] = acc;
}

// ---------------------------------------------------------------------------------
// 7. d = mean of the row's S*PER values (STOI: PER = 15 correlations per segment; ESTOI: PER = 1),
// one wave per row: lane l sums entries l, l+64, ... in order, then a fixed butterfly.  NaN
// without segments (M = 0 or fewer than 30 band frames).
// ---------------------------------------------------------------------------------
template <int PER>
__global__ __launch_bounds__(ST_THREADS) void stoi_mean_kernel(const double* __restrict__ rho,
                                                               const int* __restrict__ count,
                                                               double* __restrict__ d, int rows,
                                                               int S_max) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;   // whole waves leave
  const int n = segments(count[r]) * PER;
  const double* row = rho + (size_t)r * S_max * PER;
  double s = 0.0;
  for (int k = lane; k < n; k += 64) s += row[k];
  s = segan_wave_sum(s);
  if (lane == 0) d[r] = n > 0 ? s / n : NAN;
}

// ---------------------------------------------------------------------------------
// ESTOI 6. One wave per (segment s, row): the windows X[:, s:s+30], Y[:, s:s+30] staged in LDS
// (2 x 450 doubles per wave), then the zero rule along the rows (one lane per (band, signal),
// the 30 frames in ascending order) and along the columns of the result (one lane per (frame,
// signal), the 15 bands in ascending order), each lane rewriting its own vector in place:
//   raw = sum v^2, c = v - mean v, e = sum c^2;  v <- c / sqrt(e) if raw > 0 and e > 2^-40 raw,
//   else zeros (a degenerate vector correlates with nothing; the relative threshold keeps
//   rounding residue, 1e-32 of raw where a window's rows are all the same vector, from being
//   normalised to unit length).
// d_s = sum Xn Yn / 30: lane l sums entries l, l+64, ... in order, then the fixed butterfly.
// The four waves of a workgroup work on their own segments; waves without a segment only keep
// the barriers company.  dm: [rows][S_max].
// ---------------------------------------------------------------------------------
#define ES_WIN (ST_J * ST_SEG)
#define ES_ZERO_RULE 0x1p-40

// the zero rule on the n values v[0], v[stride], ...
__device__ __forceinline__ void estoi_normalise(double* v, int n, int stride) {
  double raw = 0.0, sum = 0.0;
  for (int k = 0; k < n; ++k) {
    const double a = v[k * stride];
    raw = fma(a, a, raw);
    sum += a;
  }
  const double mean = sum / n;
  double e = 0.0;
  for (int k = 0; k < n; ++k) {
    const double c = v[k * stride] - mean;
    e = fma(c, c, e);
  }
  const bool keep = raw > 0.0 && e > ES_ZERO_RULE * raw;
  const double norm = sqrt(e);
  for (int k = 0; k < n; ++k) v[k * stride] = keep ? (v[k * stride] - mean) / norm : 0.0;
}

__global__ __launch_bounds__(ST_THREADS) void estoi_segment_kernel(
    const double* __restrict__ X, const double* __restrict__ Y, const int* __restrict__ count,
    double* __restrict__ dm, int Fb_max, int S_max) {
  __shared__ double win[ST_THREADS / 64][2][ES_WIN];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int s = blockIdx.x * (ST_THREADS / 64) + wave;
  const int r = blockIdx.y;
  const bool active = s < S_max && s < segments(count[r]);   // wave-uniform
  double* wx = win[wave][0];
  double* wy = win[wave][1];
  if (active) {
    const size_t base = (size_t)r * ST_J * Fb_max + s;   // frames s .. s+29 < the row's F'
    for (int k = lane; k < ES_WIN; k += 64) {
      const int i = k / ST_SEG, f = k - i * ST_SEG;
      wx[k] = X[base + (size_t)i * Fb_max + f];
      wy[k] = Y[base + (size_t)i * Fb_max + f];
    }
  }
  __syncthreads();
  if (active && lane < 2 * ST_J)
    estoi_normalise((lane < ST_J ? wx : wy) + (lane % ST_J) * ST_SEG, ST_SEG, 1);
  __syncthreads();
  if (active && lane < 2 * ST_SEG)
    estoi_normalise((lane < ST_SEG ? wx : wy) + lane % ST_SEG, ST_J, ST_SEG);
  __syncthreads();
  if (!active) return;   // whole waves leave, no barrier follows
  double acc = 0.0;
  for (int k = lane; k < ES_WIN; k += 64) acc = fma(wx[k], wy[k], acc);
  acc = segan_wave_sum(acc);
  if (lane == 0) dm[(size_t)r * S_max + s] = acc / ST_SEG;
}

extern "C" int segan_stoi_plan(int srate, int* pq, int* ntaps, double* taps, int cap,
                               int* bands) {
  SEGAN_REQUIRE(pq && ntaps, "stoi_plan: NULL pointer");
  SEGAN_REQUIRE(srate_ok(srate), "stoi_plan: srate %d outside %d .. %d Hz", srate, ST_SRATE_MIN,
                ST_SRATE_MAX);
  segan_reduce_ratio(ST_FS, srate, &pq[0], &pq[1]);
  std::vector<double> g;
  segan_kaiser_sinc_taps(pq[0], pq[1], ST_ZEROS, ST_BETA, false, &g);
  *ntaps = (int)g.size();
  if (taps) {
    SEGAN_REQUIRE(cap >= *ntaps, "stoi_plan: %d taps do not fit in %d", *ntaps, cap);
    for (int n = 0; n < *ntaps; ++n) taps[n] = g[n];
  }
  if (bands) {
    BandTable bt;
    make_bands(&bt);
    for (int i = 0; i < ST_J; ++i) {
      bands[2 * i] = bt.lo[i];
      bands[2 * i + 1] = bt.hi[i];
    }
  }
  return SEGAN_OK;
}

extern "C" int segan_stoi_dims(int T, int srate, int* dims) {
  SEGAN_REQUIRE(dims, "stoi_dims: NULL pointer");
  StoiDims d;
  if (int e = stoi_dims("stoi_dims", T, srate, &d)) return e;
  dims[0] = d.Ly;
  dims[1] = d.F;
  dims[2] = d.Lc;
  dims[3] = d.Fb;
  dims[4] = d.S;
  return SEGAN_OK;
}

// Stages 1-5 of both measures: argument checks, then resample -> frame energies -> select ->
// compaction -> band envelopes on `st`.  `last`, `d`: the caller's last-stage buffers, checked
// here so that every check precedes the first launch.  dims: the stage sizes for T.
static int stoi_front(const char* what, const float* ref, const float* deg, const int* lengths,
                      int rows, int T, int srate, double* xr, double* yr, double* energy,
                      int* mask, int* kept, int* count, double* xs, double* ys, double* X,
                      double* Y, const void* last, const void* d, StoiDims* dims, hipStream_t st) {
  SEGAN_REQUIRE(ref && deg && xr && yr && energy && mask && kept && count && xs && ys && X && Y &&
                    last && d,
                "%s: NULL pointer", what);
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && T > 0, "%s: bad sizes rows=%d T=%d", what, rows, T);
  StoiDims& dm = *dims;
  if (int e = stoi_dims(what, T, srate, &dm)) return e;
  const StoiTables* tb = get_tables(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const dim3 blk(ST_THREADS);
  const float* in[2] = {ref, deg};
  double* out[2] = {xr, yr};
  for (int i = 0; i < 2; ++i)
    if (int e = segan_resample_rows(tb->p, tb->q, ST_ZEROS, ST_BETA, false, in[i], SEGAN_DT_F32,
                                    lengths, rows, T, out[i], SEGAN_DT_F64, dm.Ly, nullptr,
                                    nullptr, st))
      return e;
  if (dm.F > 0)
    hipLaunchKernelGGL(stoi_energy_kernel, dim3(ceil_div(dm.F, ST_THREADS / 64), rows), blk, 0, st,
                       xr, lengths, energy, T, dm.Ly, dm.F, tb->p, tb->q, tb->window);
  hipLaunchKernelGGL(stoi_select_kernel, dim3(rows), blk, 0, st, energy, lengths, mask, kept, count,
                     T, dm.F, tb->p, tb->q);
  if (dm.Lc > 0)
    hipLaunchKernelGGL(stoi_compact_kernel, dim3(ceil_div(dm.Lc, ST_THREADS), rows, 2), blk, 0, st,
                       xr, yr, kept, count, xs, ys, dm.Ly, dm.F, dm.Lc, tb->window);
  if (dm.Fb > 0)
    hipLaunchKernelGGL(stoi_band_kernel, dim3(dm.Fb, rows), blk, 0, st, xs, ys, count, X, Y, dm.Lc,
                       dm.Fb, tb->klo, tb->nb, tb->bands, tb->window, tb->tw);
  return SEGAN_OK;
}

extern "C" int segan_stoi(const float* ref, const float* deg, const int* lengths, int rows, int T,
                          int srate, double* xr, double* yr, double* energy, int* mask, int* kept,
                          int* count, double* xs, double* ys, double* X, double* Y, double* rho,
                          double* d, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  StoiDims dm;
  if (int e = stoi_front("stoi", ref, deg, lengths, rows, T, srate, xr, yr, energy, mask, kept,
                         count, xs, ys, X, Y, rho, d, &dm, st))
    return e;
  const dim3 blk(ST_THREADS);
  if (dm.S > 0)
    hipLaunchKernelGGL(stoi_segment_kernel, dim3(ceil_div(dm.S * ST_J, ST_THREADS), rows), blk, 0,
                       st, X, Y, count, rho, dm.Fb, dm.S, pow(10.0, 15.0 / 20.0));
  hipLaunchKernelGGL(stoi_mean_kernel<ST_J>, dim3(ceil_div(rows, ST_THREADS / 64)), blk, 0, st, rho,
                     count, d, rows, dm.S);
  return segan_check_launch("stoi");
}

extern "C" int segan_estoi(const float* ref, const float* deg, const int* lengths, int rows, int T,
                           int srate, double* xr, double* yr, double* energy, int* mask, int* kept,
                           int* count, double* xs, double* ys, double* X, double* Y, double* dseg,
                           double* d, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  StoiDims dm;
  if (int e = stoi_front("estoi", ref, deg, lengths, rows, T, srate, xr, yr, energy, mask, kept,
                         count, xs, ys, X, Y, dseg, d, &dm, st))
    return e;
  const dim3 blk(ST_THREADS);
  if (dm.S > 0)
    hipLaunchKernelGGL(estoi_segment_kernel, dim3(ceil_div(dm.S, ST_THREADS / 64), rows), blk, 0,
                       st, X, Y, count, dseg, dm.Fb, dm.S);
  hipLaunchKernelGGL(stoi_mean_kernel<1>, dim3(ceil_div(rows, ST_THREADS / 64)), blk, 0, st, dseg,
                     count, d, rows, dm.S);
  return segan_check_launch("estoi");
}
