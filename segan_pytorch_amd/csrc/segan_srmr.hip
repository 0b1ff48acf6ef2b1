// SRMR, the speech-to-reverberation modulation energy ratio of Falk, Zheng and Chan (2010), and the
// batched power-of-two complex fp64 FFT its Hilbert envelope needs.  fp64
// on fp32 rows with per-row lengths, no atomics, every sum and every recurrence in an order fixed
// by the sample index alone: a row's bits depend neither on T, nor on the other rows, nor on the
// samples past its length, nor on how the caller chunks the batch.
//
//   fft_kernel            radix-2 Stockham passes on up to 4096 complex doubles in LDS: one
//                         transform, or 2^b interleaved ones (the columns or rows of a two-level
//                         transform, or short transforms of a batch); twiddle, analytic mask, 1/n
//                         and magnitude are applied on the way out
//                         (the passes themselves and the twiddle table: segan_fft_lds.h, shared
//                         with segan_dereverb.hip)
//   srmr_gammatone_kernel one lane per (row, channel): four cascaded biquads over the row's
//                         samples into the complex work buffer, zero-padded to the row's own L
//   srmr_modulation_kernel  one lane per (row, channel, band): the band-pass over the envelope
//                         and the windowed squares of the (at most four) frames a sample is in
//   srmr_final_kernel     one workgroup per row: frame means, shares, BW, K*, the ratio
#include "segan_fft_lds.h"

#define SRMR_CH SEGAN_SRMR_CHANNELS
#define SRMR_BANDS SEGAN_SRMR_BANDS
#define SRMR_PAIRS (SRMR_CH * SRMR_BANDS)
#define SRMR_OVERLAP 4                           // wl / wi: the frames a sample belongs to
#define SRMR_BLOCK 16       // samples whose loads the gammatone lane issues at once
#define SRMR_MOD_BLOCK 8    // and the modulation lane

static_assert(SEGAN_FFT_MAX_LOG2 <= 2 * FFT_LDS_LOG2, "fft: two levels reach the largest size");
static_assert(SEGAN_SRMR_STAGE == 2 * SRMR_CH + SRMR_PAIRS + 4, "srmr: the stage block");

namespace {

enum { FFT_SINGLE = 0, FFT_COL, FFT_COLT, FFT_ROW, FFT_ROWT };

// One launch of fft_kernel.  n = 2^lg <= 4096 is one transform in LDS (FFT_SINGLE).  Above that
// n = N1 N2, N1 = 2^(lg / 2): the columns (length N1, stride N2) are transformed and multiplied by
// w_n^(k1 n2) (FFT_COL in place, FFT_COLT into the transposed position k1 + N1 n2), then the rows
// (length N2: FFT_ROW contiguous and in place, which leaves X[k1 + N1 k2] at k1 N2 + k2;
// FFT_ROWT on the transposed layout and in place, which leaves the natural order).
struct FftGeom {
  int lgsub, lgbatch;        // the transform in LDS and how many of them are interleaved there
  long long ld_i, ld_t;      // element i of transform t is read at i ld_i + t ld_t
  long long st_k, st_t;      // and output k is written at k st_k + t st_t
  long long tcount;          // transforms (columns, rows) of this level
  bool ld_ifast, st_kfast;   // which index runs along memory
  long long bin_k, bin_t;    // the frequency bin of output (k, t) of the last level
};

__host__ __device__ inline int fft_ceil_log2(long long n) {
  int lg = 0;
  while ((1LL << lg) < n) ++lg;
  return lg;
}

__host__ __device__ inline FftGeom fft_geom(int lg, int kind, long long ntrans) {
  FftGeom g;
  const int lg1 = lg / 2, lg2 = lg - lg1;
  const long long N1 = 1LL << lg1, N2 = 1LL << lg2;
  g.bin_k = 1;
  g.bin_t = 0;
  if (kind == FFT_SINGLE) {
    g.lgsub = lg;
    g.lgbatch = FFT_LDS_LOG2 - lg;
    while (g.lgbatch > 0 && (1LL << (g.lgbatch - 1)) >= ntrans) --g.lgbatch;
    g.ld_i = g.st_k = 1;
    g.ld_t = g.st_t = 1LL << lg;
    g.tcount = ntrans;
    g.ld_ifast = g.st_kfast = true;
  } else if (kind == FFT_COL || kind == FFT_COLT) {
    g.lgsub = lg1;
    g.lgbatch = FFT_LDS_LOG2 - lg1;
    g.ld_i = N2;
    g.ld_t = 1;
    g.tcount = N2;
    g.ld_ifast = false;
    g.st_k = kind == FFT_COL ? N2 : 1;
    g.st_t = kind == FFT_COL ? 1 : N1;
    g.st_kfast = kind == FFT_COLT;
  } else if (kind == FFT_ROW) {
    g.lgsub = lg2;
    g.lgbatch = FFT_LDS_LOG2 - lg2;
    g.ld_i = g.st_k = 1;
    g.ld_t = g.st_t = N2;
    g.tcount = N1;
    g.ld_ifast = g.st_kfast = true;
    g.bin_k = N1;
    g.bin_t = 1;
  } else {
    g.lgsub = lg2;
    g.lgbatch = FFT_LDS_LOG2 - lg2;
    g.ld_i = g.st_k = N1;
    g.ld_t = g.st_t = 1;
    g.tcount = N1;
    g.ld_ifast = g.st_kfast = false;
    g.bin_k = N1;
    g.bin_t = 1;
  }
  return g;
}

inline long long fft_tiles(int lg, int kind, long long ntrans) {
  const FftGeom g = fft_geom(lg, kind, ntrans);
  const long long batch = 1LL << g.lgbatch;
  return (g.tcount + batch - 1) / batch;
}

struct FftArgs {
  const double2* in;
  double2* out;
  const double2* tw;       // (cos, sin)(2 pi m / 4096), m < 2048
  long long ostride;       // complex values between the transforms of consecutive workgroup rows
  long long ntrans;        // FFT_SINGLE: the transforms of one workgroup row, n apart
  int tiles;               // workgroups per workgroup row
  int lg;                  // log2 n (plain mode)
  int kind, inverse, twiddle, mask, scale, mag;
  // srmr mode (phase > 0): workgroup row = (row, channel), n is the row's own L and the launch's
  // role follows from it (srmr_phase)
  int phase;
  const int* lengths;
  int T, wl;
};

// The envelope's four launches.  n <= 4096: forward + mask (phase 1), inverse + 1/n + magnitude
// (phase 3).  Above: columns + twiddle (1), rows + mask (2), inverse rows + twiddle (3), inverse
// columns + 1/n + magnitude (4): the spectrum stays in the permuted order in between, so every
// launch is in place.
__device__ inline bool srmr_phase(int lg, FftArgs* a) {
  const bool small = lg <= FFT_LDS_LOG2;
  if (small && (a->phase == 2 || a->phase == 4)) return false;
  a->lg = lg;
  a->ntrans = 1;
  a->inverse = a->phase >= 3;
  if (small) {
    a->kind = FFT_SINGLE;
    a->mask = a->phase == 1;
    a->scale = a->mag = a->phase == 3;
    a->twiddle = 0;
  } else {
    a->kind = (a->phase == 1 || a->phase == 4) ? FFT_COL : FFT_ROW;
    a->twiddle = a->phase == 1 || a->phase == 3;
    a->mask = a->phase == 2;
    a->scale = a->mag = a->phase == 4;
  }
  return true;
}

__global__ __launch_bounds__(FFT_THREADS) void fft_kernel(FftArgs a) {
  __shared__ double2 sm[FFT_LDS_N];
  const int tid = threadIdx.x;
  const long long wrow = blockIdx.x / a.tiles;
  const int tile = blockIdx.x % a.tiles;
  if (a.phase > 0) {
    const int N = segan_row_samples(a.lengths, (int)(wrow / SRMR_CH), a.T);
    if (N < a.wl) return;                               // the whole workgroup, before any barrier
    if (!srmr_phase(fft_ceil_log2(N), &a)) return;
  }
  const FftGeom g = fft_geom(a.lg, a.kind, a.ntrans);
  const long long t0 = (long long)tile << g.lgbatch;
  if (t0 >= g.tcount) return;
  const int M = 1 << (g.lgsub + g.lgbatch);
  const int sub_mask = (1 << g.lgsub) - 1, batch_mask = (1 << g.lgbatch) - 1;
  const double2* in = a.in + wrow * a.ostride;
  double2* out = a.out + wrow * a.ostride;

  for (int idx = tid; idx < M; idx += FFT_THREADS) {
    const int i = g.ld_ifast ? (idx & sub_mask) : (idx >> g.lgbatch);
    const int t = g.ld_ifast ? (idx >> g.lgsub) : (idx & batch_mask);
    const long long tg = t0 + t;
    sm[(i << g.lgbatch) | t] =
        tg < g.tcount ? in[i * g.ld_i + tg * g.ld_t] : make_double2(0.0, 0.0);
  }
  __syncthreads();

  fft_lds_passes(sm, a.tw, g.lgsub, g.lgbatch, a.inverse != 0);

  const long long n = 1LL << a.lg;
  const double inv_n = 1.0 / (double)n;
  for (int idx = tid; idx < M; idx += FFT_THREADS) {
    const int k = g.st_kfast ? (idx & sub_mask) : (idx >> g.lgbatch);
    const int t = g.st_kfast ? (idx >> g.lgsub) : (idx & batch_mask);
    const long long tg = t0 + t;
    if (tg >= g.tcount) continue;
    double2 v = sm[(k << g.lgbatch) | t];
    if (a.twiddle) {
      double s, c;
      sincospi(2.0 * (double)(k * tg) * inv_n, &s, &c);   // k tg < n: the argument is exact
      if (!a.inverse) s = -s;
      v = cmul(v.x, v.y, c, s);
    }
    if (a.mask) {   // the analytic signal: bins 0 and n/2 kept, below n/2 doubled, above zeroed
      const long long bin = k * g.bin_k + tg * g.bin_t;
      const double f = (bin == 0 || bin == n / 2) ? 1.0 : (bin < n / 2 ? 2.0 : 0.0);
      v.x *= f;
      v.y *= f;
    }
    if (a.scale) {
      v.x *= inv_n;
      v.y *= inv_n;
    }
    if (a.mag) v = make_double2(sqrt(fma(v.x, v.x, v.y * v.y)), 0.0);
    out[k * g.st_k + tg * g.st_t] = v;
  }
}

// ---- tables ----

// doubles of the per-rate table: gammatone [23][10] (b0, b1 of the four sections in running
// order, a1, a2), modulation [8][4] (b0, b2, a1, a2, all over a0), cutoffs [8], cfs [23],
// erbs [23], the window [wl]
#define SRMR_GT_COEF 10
#define SRMR_MOD_COEF 4
#define SRMR_OFF_MOD (SRMR_CH * SRMR_GT_COEF)
#define SRMR_OFF_CUT (SRMR_OFF_MOD + SRMR_BANDS * SRMR_MOD_COEF)
#define SRMR_OFF_CF (SRMR_OFF_CUT + SRMR_BANDS)
#define SRMR_OFF_ERB (SRMR_OFF_CF + SRMR_CH)
#define SRMR_OFF_WIN (SRMR_OFF_ERB + SRMR_CH)

struct SrmrTable {
  int device;
  int rate;
  double* d;
};
SeganDeviceTables<SrmrTable> g_srmr_tables;

inline int srmr_wl(int rate) { return (int)ceil(0.256 * rate); }
inline int srmr_wi(int rate) { return (int)ceil(0.064 * rate); }

// The constants of scripts/srmr_oracle.py, operation by operation (no contraction: the centre
// frequencies and the bandwidths are compared bit for bit).
void srmr_constants(int rate, std::vector<double>* out) {
#pragma clang fp contract(off)
  const double fs = rate, T = 1.0 / fs, high = fs / 2.0;
  const double earq = 9.26449, minbw = 24.7, low = 125.0, c0 = earq * minbw;
  const int wl = srmr_wl(rate);
  std::vector<double>& v = *out;
  v.assign(SRMR_OFF_WIN + wl, 0.0);
  const double dlog = log(low + c0) - log(high + c0);
  const double r1 = sqrt(3.0 + pow(2.0, 1.5)), r2 = sqrt(3.0 - pow(2.0, 1.5));
  for (int i = 0; i < SRMR_CH; ++i) {
    const double cf = -c0 + exp((double)(i + 1) * dlog / SRMR_CH) * (high + c0);
    const double erb = cf / earq + minbw;
    v[SRMR_OFF_CF + i] = cf;
    v[SRMR_OFF_ERB + i] = erb;
    const double B = 1.019 * 2.0 * M_PI * erb;
    const double c = cos(2.0 * M_PI * cf * T), s = sin(2.0 * M_PI * cf * T), g = exp(-B * T);
    const double a1 = -2.0 * c * g, a2 = g * g;
    double* q = &v[i * SRMR_GT_COEF];
    const double sign[4] = {1.0, -1.0, 1.0, -1.0}, root[4] = {r1, r1, r2, r2};
    // z^-1 at the centre frequency and the cascade's response there, in double pairs
    const double zr = cos(2.0 * M_PI * cf * T), zi = -sin(2.0 * M_PI * cf * T);
    const double z2r = zr * zr - zi * zi, z2i = 2.0 * zr * zi;
    const double dr = 1.0 + a1 * zr + a2 * z2r, di = a1 * zi + a2 * z2i;
    double hr = 1.0, hi = 0.0;
    for (int j = 0; j < 4; ++j) {
      q[2 * j] = T;
      q[2 * j + 1] = -(2.0 * T * c * g + sign[j] * 2.0 * root[j] * T * s * g) / 2.0;
      const double nr = q[2 * j] + q[2 * j + 1] * zr, ni = q[2 * j + 1] * zi;
      const double dd = dr * dr + di * di;
      const double fr = (nr * dr + ni * di) / dd, fi = (ni * dr - nr * di) / dd;
      const double tr = hr * fr - hi * fi, ti = hr * fi + hi * fr;
      hr = tr;
      hi = ti;
    }
    const double gain = hypot(hr, hi);
    q[0] /= gain;
    q[1] /= gain;
    q[8] = a1;
    q[9] = a2;
  }
  for (int k = 0; k < SRMR_BANDS; ++k) {
    const double f = 4.0 * pow(32.0, (double)k / 7.0);
    const double W = tan(M_PI * f / fs), B0 = W / 2.0;
    const double a0 = 1.0 + B0 + W * W;
    double* q = &v[SRMR_OFF_MOD + k * SRMR_MOD_COEF];
    q[0] = B0 / a0;
    q[1] = -B0 / a0;
    q[2] = (2.0 * W * W - 2.0) / a0;
    q[3] = (1.0 - B0 + W * W) / a0;
    v[SRMR_OFF_CUT + k] = f - B0 * fs / (2.0 * M_PI);
  }
  for (int n = 0; n < wl; ++n)
    v[SRMR_OFF_WIN + n] = 0.54 - 0.46 * cos(2.0 * M_PI * (double)n / (double)wl);
}

const SrmrTable* srmr_table(int rate) {
  return g_srmr_tables.get(
      "srmr", [rate](const SrmrTable& e) { return e.rate == rate; },
      [rate](SrmrTable* e) {
        std::vector<double> v;
        srmr_constants(rate, &v);
        e->rate = rate;
        return segan_upload(&e->d, v, "srmr");
      });
}

// ---- SRMR ----

// y = z0 + b0 x; z0 = z1 + b1 x - a1 y; z1 = b2 x - a2 y: the transposed direct form II of
// scipy.signal.lfilter, the order of the oracle
struct Biquad {
  double z0, z1;
};

// One lane per (row, channel), sequential in time: the recurrence in the oracle's own order, so
// the only difference to it is that a multiply and the add after it round once (explicit fma).
// Y[(row, channel)][t] = (y, 0) for t < N and zero up to the row's own L.
__global__ __launch_bounds__(64) void srmr_gammatone_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, int rows, int T, int wl,
    long long Lmax, const double* __restrict__ tab, double2* __restrict__ Y) {
  const long long pair = (long long)blockIdx.x * 64 + threadIdx.x;
  if (pair >= (long long)rows * SRMR_CH) return;
  const int row = (int)(pair / SRMR_CH), ch = (int)(pair % SRMR_CH);
  const int N = segan_row_samples(lengths, row, T);
  if (N < wl) return;
  const long long L = 1LL << fft_ceil_log2(N);
  const double* q = tab + ch * SRMR_GT_COEF;
  double b0[4], b1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    b0[j] = q[2 * j];
    b1[j] = q[2 * j + 1];
  }
  const double a1 = q[8], a2 = q[9];
  Biquad s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j].z0 = s[j].z1 = 0.0;
  const float* xr = x + (size_t)row * T;
  double2* y = Y + pair * Lmax;
  auto step = [&](float xin) {
    double v = (double)xin;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double o = fma(b0[j], v, s[j].z0);
      s[j].z0 = fma(-a1, o, fma(b1[j], v, s[j].z1));
      s[j].z1 = -(a2 * o);
      v = o;
    }
    return v;
  };
  // the loads of a block are issued together: their latency is paid once per block, not per step
  int t = 0;
  for (; t + SRMR_BLOCK <= N; t += SRMR_BLOCK) {
    float xs[SRMR_BLOCK];
#pragma unroll
    for (int u = 0; u < SRMR_BLOCK; ++u) xs[u] = xr[t + u];
#pragma unroll
    for (int u = 0; u < SRMR_BLOCK; ++u) y[t + u] = make_double2(step(xs[u]), 0.0);
  }
  for (; t < N; ++t) y[t] = make_double2(step(xr[t]), 0.0);
  for (long long z = N; z < L; ++z) y[z] = make_double2(0.0, 0.0);
}

// One lane per (row, channel, band), the eight bands of a pair in consecutive lanes (they read
// the same envelope sample).  The lane keeps its biquad state and the running sums of the four
// frames the sample is in: in the segment g of wi samples these are the frames g .. g - 3, at
// window offsets 0, wi, 2 wi, 3 wi; after a full segment g the frame g - 3 is complete and is
// written, the sums move up.  Lane band 0 also sums e^2 over the N samples.
__global__ __launch_bounds__(64) void srmr_modulation_kernel(
    const int* __restrict__ lengths, int rows, int T, int wl, int wi, long long Lmax, int nfmax,
    const double* __restrict__ tab, const double2* __restrict__ Y, double* __restrict__ E,
    double* __restrict__ EE) {
  const long long gid = (long long)blockIdx.x * 64 + threadIdx.x;
  if (gid >= (long long)rows * SRMR_PAIRS) return;
  const long long pair = gid / SRMR_BANDS;
  const int band = (int)(gid % SRMR_BANDS), row = (int)(pair / SRMR_CH);
  const int N = segan_row_samples(lengths, row, T);
  if (N < wl) return;
  const int nf = 1 + (N - wl) / wi;
  const double* q = tab + SRMR_OFF_MOD + band * SRMR_MOD_COEF;
  const double b0 = q[0], b2 = q[1], a1 = q[2], a2 = q[3];
  const double* w = tab + SRMR_OFF_WIN;
  const double2* e = Y + pair * Lmax;
  double* Ef = E + gid * nfmax;
  double acc[SRMR_OVERLAP] = {0.0, 0.0, 0.0, 0.0};
  double z0 = 0.0, z1 = 0.0, ee = 0.0;
  for (int g = 0, base = 0; base < N; ++g, base += wi) {
    const int cnt = N - base < wi ? N - base : wi;
    auto step = [&](double v, const double (&wv)[SRMR_OVERLAP]) {
      ee = fma(v, v, ee);
      const double m = fma(b0, v, z0);
      z0 = fma(-a1, m, z1);
      z1 = fma(-a2, m, b2 * v);
#pragma unroll
      for (int j = 0; j < SRMR_OVERLAP; ++j) {
        const double wm = wv[j] * m;
        acc[j] = fma(wm, wm, acc[j]);
      }
    };
    int u = 0;
    for (; u + SRMR_MOD_BLOCK <= cnt; u += SRMR_MOD_BLOCK) {   // loads first, as in the gammatone
      double vs[SRMR_MOD_BLOCK], ws[SRMR_MOD_BLOCK][SRMR_OVERLAP];
#pragma unroll
      for (int i = 0; i < SRMR_MOD_BLOCK; ++i) {
        vs[i] = e[base + u + i].x;
#pragma unroll
        for (int j = 0; j < SRMR_OVERLAP; ++j) ws[i][j] = w[j * wi + u + i];
      }
#pragma unroll
      for (int i = 0; i < SRMR_MOD_BLOCK; ++i) step(vs[i], ws[i]);
    }
    for (; u < cnt; ++u) {
      const double wv[SRMR_OVERLAP] = {w[u], w[wi + u], w[2 * wi + u], w[3 * wi + u]};
      step(e[base + u].x, wv);
    }
    const int f = g - (SRMR_OVERLAP - 1);
    if (cnt == wi && f >= 0 && f < nf) Ef[f] = acc[SRMR_OVERLAP - 1];
#pragma unroll
    for (int j = SRMR_OVERLAP - 1; j > 0; --j) acc[j] = acc[j - 1];
    acc[0] = 0.0;
  }
  if (band == 0) EE[pair] = ee;
}

// One workgroup per row.  Thread (i, k): Ebar[i][k] = (sum over the frames in ascending order) /
// n_frames.  Thread 0 then walks the 184 means in index order: total, shares cumulated from the
// lowest centre frequency (the last channel) upwards, BW, K*, the ratio.  A row shorter than one
// frame or without energy is NaN.  stage[row] = cfs[23], envelope_energy[23], Ebar[23][8], bw,
// kstar, share, srmr.
__global__ __launch_bounds__(FFT_THREADS) void srmr_final_kernel(
    const int* __restrict__ lengths, int T, int wl, int wi, int nfmax,
    const double* __restrict__ tab, const double* __restrict__ E, const double* __restrict__ EE,
    double* __restrict__ stage, double* __restrict__ row_out) {
  __shared__ double eb[SRMR_PAIRS];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int N = segan_row_samples(lengths, row, T);
  const int nf = N < wl ? 0 : 1 + (N - wl) / wi;
  double* sg = stage + (size_t)row * SEGAN_SRMR_STAGE;
  if (tid < SRMR_PAIRS) {
    double acc = 0.0;
    const double* p = E + ((size_t)row * SRMR_PAIRS + tid) * nfmax;
    for (int f = 0; f < nf; ++f) acc += p[f];
    const double mean = nf > 0 ? acc / (double)nf : 0.0;
    eb[tid] = mean;
    sg[2 * SRMR_CH + tid] = mean;
  }
  if (tid < SRMR_CH) {
    sg[tid] = tab[SRMR_OFF_CF + tid];
    sg[SRMR_CH + tid] = nf > 0 ? EE[(size_t)row * SRMR_CH + tid] : 0.0;
  }
  __syncthreads();
  if (tid != 0) return;
  double total = 0.0;
  for (int j = 0; j < SRMR_PAIRS; ++j) total += eb[j];
  double bw = NAN, share = NAN, value = NAN;
  int kstar = 0;
  if (nf > 0 && total > 0.0) {
    double cum = 0.0;
    bw = tab[SRMR_OFF_ERB];
    for (int i = SRMR_CH - 1; i >= 0; --i) {
      double pc = 0.0;
      for (int k = 0; k < SRMR_BANDS; ++k) pc += eb[i * SRMR_BANDS + k];
      cum += 100.0 * pc / total;
      if (cum > 90.0) {
        bw = tab[SRMR_OFF_ERB + i];
        share = cum;
        break;
      }
    }
    const double* c = tab + SRMR_OFF_CUT;
    kstar = bw > c[7] ? 8 : (c[6] < bw && bw < c[7]) ? 7 : (c[5] < bw && bw < c[6]) ? 6 : 5;
    double num = 0.0, den = 0.0;
    for (int i = 0; i < SRMR_CH; ++i) {
      for (int k = 0; k < 4; ++k) num += eb[i * SRMR_BANDS + k];
      for (int k = 4; k < kstar; ++k) den += eb[i * SRMR_BANDS + k];
    }
    value = num / den;
  }
  sg[2 * SRMR_CH + SRMR_PAIRS] = bw;
  sg[2 * SRMR_CH + SRMR_PAIRS + 1] = (double)kstar;
  sg[2 * SRMR_CH + SRMR_PAIRS + 2] = share;
  sg[2 * SRMR_CH + SRMR_PAIRS + 3] = value;
  row_out[row] = value;
}

bool srmr_sizes_ok(int rows, int T, int rate) {
  return rows > 0 && rows <= 65535 && T > 0 && T <= (1 << SEGAN_FFT_MAX_LOG2) &&
         (rate == 8000 || rate == 16000);
}

struct SrmrDims {
  long long L, nf, per_row;
};

SrmrDims srmr_dims(int T, int rate) {
  const int wl = srmr_wl(rate), wi = srmr_wi(rate);
  SrmrDims d;
  d.L = 1LL << fft_ceil_log2(T);
  d.nf = T < wl ? 0 : 1 + (T - wl) / wi;
  // Y [23][L] complex, E [23][8][nf], EE [23], the stage block
  d.per_row = 2 * SRMR_CH * d.L + SRMR_PAIRS * d.nf + SRMR_CH + SEGAN_SRMR_STAGE;
  return d;
}

int launch_fft(const FftArgs& a, long long wrows, hipStream_t st) {
  const long long blocks = wrows * a.tiles;
  if (blocks <= 0 || blocks > 0x7fffffffLL) {
    segan_set_error("fft: %lld workgroups do not fit one launch", blocks);
    return SEGAN_EINVAL;
  }
  hipLaunchKernelGGL(fft_kernel, dim3((unsigned)blocks), dim3(FFT_THREADS), 0, st, a);
  return segan_check_launch("fft_kernel");
}

}  // namespace

extern "C" int segan_fft_z2z(const double* in, double* out, int rows, int log2n, int inverse,
                             void* stream) {
  SEGAN_REQUIRE(in && out, "fft: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && log2n >= 1 && log2n <= SEGAN_FFT_MAX_LOG2,
                "fft: bad sizes rows=%d log2n=%d", rows, log2n);
  SEGAN_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0,
                "fft: in and out must be 16-byte aligned");
  SEGAN_REQUIRE(log2n <= FFT_LDS_LOG2 || in != out,
                "fft: in place only up to n = %d", FFT_LDS_N);
  const FftTable* tab = fft_table();
  if (!tab) return SEGAN_ELAUNCH;
  FftArgs a = {};
  a.tw = tab->tw;
  a.lg = log2n;
  a.inverse = inverse != 0;
  hipStream_t st = (hipStream_t)stream;
  if (log2n <= FFT_LDS_LOG2) {
    a.in = reinterpret_cast<const double2*>(in);
    a.out = reinterpret_cast<double2*>(out);
    a.kind = FFT_SINGLE;
    a.ntrans = rows;
    a.tiles = (int)fft_tiles(log2n, FFT_SINGLE, rows);
    a.scale = a.inverse;
    return launch_fft(a, 1, st);
  }
  a.ostride = 1LL << log2n;
  a.ntrans = 1;
  a.in = reinterpret_cast<const double2*>(in);
  a.out = reinterpret_cast<double2*>(out);
  a.kind = FFT_COLT;
  a.twiddle = 1;
  a.tiles = (int)fft_tiles(log2n, FFT_COLT, 1);
  if (int e = launch_fft(a, rows, st)) return e;
  a.in = a.out;
  a.kind = FFT_ROWT;
  a.twiddle = 0;
  a.scale = a.inverse;
  a.tiles = (int)fft_tiles(log2n, FFT_ROWT, 1);
  return launch_fft(a, rows, st);
}

extern "C" int segan_srmr_dims(int rows, int T, int rate, long long* out) {
  SEGAN_REQUIRE(out, "srmr: NULL pointer");
  SEGAN_REQUIRE(srmr_sizes_ok(rows, T, rate), "srmr: bad sizes rows=%d T=%d rate=%d", rows, T,
                rate);
  const SrmrDims d = srmr_dims(T, rate);
  out[0] = d.L;
  out[1] = d.nf;
  out[2] = d.per_row;
  out[3] = d.per_row * rows;
  return SEGAN_OK;
}

extern "C" int segan_srmr(const float* x, const int* lengths, int rows, int T, int rate,
                          double* row_out, double* stages_out, double* ws, void* stream) {
  SEGAN_REQUIRE(x && row_out && ws, "srmr: NULL pointer");
  SEGAN_REQUIRE(srmr_sizes_ok(rows, T, rate), "srmr: bad sizes rows=%d T=%d rate=%d", rows, T,
                rate);
  SEGAN_REQUIRE(((uintptr_t)ws & 15) == 0, "srmr: the workspace must be 16-byte aligned");
  const int wl = srmr_wl(rate), wi = srmr_wi(rate);
  SEGAN_REQUIRE(wl == SRMR_OVERLAP * wi, "srmr: frames of %d every %d samples", wl, wi);
  const SrmrDims d = srmr_dims(T, rate);
  const FftTable* ft = fft_table();
  const SrmrTable* tab = srmr_table(rate);
  if (!ft || !tab) return SEGAN_ELAUNCH;
  hipStream_t st = (hipStream_t)stream;
  const int nfmax = (int)d.nf;
  double2* Y = reinterpret_cast<double2*>(ws);                     // [rows][23][L]
  double* E = ws + 2 * (size_t)rows * SRMR_CH * d.L;               // [rows][23][8][nf]
  double* EE = E + (size_t)rows * SRMR_PAIRS * nfmax;              // [rows][23]
  double* stage = stages_out ? stages_out : EE + (size_t)rows * SRMR_CH;

  if (nfmax > 0) {   // else no row has a full frame: every row is NaN
    const long long pairs = (long long)rows * SRMR_CH;
    hipLaunchKernelGGL(srmr_gammatone_kernel, dim3((unsigned)((pairs + 63) / 64)), dim3(64), 0,
                       st, x, lengths, rows, T, wl, d.L, (const double*)tab->d, Y);
    if (int e = segan_check_launch("srmr_gammatone_kernel")) return e;
    const int lgmin = fft_ceil_log2(wl), lgmax = fft_ceil_log2(T);
    for (int phase = 1; phase <= 4; ++phase) {
      if (lgmax <= FFT_LDS_LOG2 && (phase == 2 || phase == 4)) continue;
      FftArgs a = {};
      a.in = Y;
      a.out = Y;
      a.tw = ft->tw;
      a.ostride = d.L;
      a.phase = phase;
      a.lengths = lengths;
      a.T = T;
      a.wl = wl;
      long long tiles = 1;   // the most workgroups any row's own L needs in this phase
      for (int lg = lgmin > FFT_LDS_LOG2 ? lgmin : FFT_LDS_LOG2 + 1; lg <= lgmax; ++lg) {
        const long long t = fft_tiles(lg, (phase == 1 || phase == 4) ? FFT_COL : FFT_ROW, 1);
        if (t > tiles) tiles = t;
      }
      a.tiles = (int)tiles;
      if (int e = launch_fft(a, pairs, st)) return e;
    }
    const long long lanes = pairs * SRMR_BANDS;
    hipLaunchKernelGGL(srmr_modulation_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0,
                       st, lengths, rows, T, wl, wi, d.L, nfmax, (const double*)tab->d,
                       (const double2*)Y, E, EE);
    if (int e = segan_check_launch("srmr_modulation_kernel")) return e;
  }
  hipLaunchKernelGGL(srmr_final_kernel, dim3(rows), dim3(FFT_THREADS), 0, st, lengths, T, wl, wi,
                     nfmax, (const double*)tab->d, (const double*)E, (const double*)EE, stage,
                     row_out);
  return segan_check_launch("srmr_final_kernel");
}
