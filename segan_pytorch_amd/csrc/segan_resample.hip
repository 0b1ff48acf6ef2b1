// segan_resample.hip — sample-rate conversion of rows of audio by a rational factor p / q =
// rate_out / rate_in (lowest terms), fp64 throughout (DESIGN.md section 12 states the rules; the
// numpy oracle is scripts/resample_oracle.py).  The filter is scipy.signal.resample_poly's:
//   mx = max(p, q), lh = zeros mx, h[t] = sinc(t / mx) kaiser(2 lh + 1, beta)[t + lh], t = -lh..lh,
//   G[t] = p h[t] / sum(h);   y[m] = sum_n x[n] G[m q - n p] over |m q - n p| <= lh, 0 <= n < Lx,
// ascending n, m = 0 .. ceil(Lx p / q) - 1.  (zeros, beta) = (10, 5.0) is scipy's default filter
// and, towards 10 kHz, STOI's.
//
// This file holds the one resampling kernel and the one filter designer of the library.
// segan_resample and segan_stoi (stage 1, twice: clean and processed) both go through
// segan_resample_rows; segan_resample_plan and segan_stoi_plan both go through
// segan_kaiser_sinc_taps.  The designer has two normalisation modes because the two users are
// pinned to different things: STOI to its oracle's index-order sum of h at every rate from 4 to
// 48 kHz, the public converter to 1e-15 of the exactly normalised filter, which the index-order
// sum misses at some ratios (11025 and 37800 -> 10000 Hz among them).  Where it does not, the
// two modes give the same bits.
//
// One workgroup per (row, tile of RS_TILE outputs).  The input span the tile reads is staged in
// LDS as doubles, RS_CHUNK samples per pass (one pass unless rate_in / rate_out or zeros is
// large); every thread owns one output and adds its products in ascending n across the passes,
// so the sum does not depend on the tile, the chunking or the other rows.
//
// Taps: output m reads phase (m q) mod p of the filter, K = 2 lh / p + 1 taps at most.  The table
// is stored transposed and in VISITING order, tab[j p + s] with s = m mod p: at step j of the
// tap loop the 64 lanes of a wave (consecutive m) read consecutive doubles (one wrap at p), so a
// wave's reads fall in 4 or 5 cache lines whatever q is; with p == 1 every lane reads the same
// double.  Tables of at most RS_TAPS_LDS doubles (48 -> 16 kHz and 16 -> 48 kHz at zeros = 32:
// 193 and 195) are copied to LDS per workgroup; larger ones (160 / 441 at zeros = 32: 28 320
// doubles, 2469 / 3200: 204 927) are read through L2.  Built on the host and uploaded once per
// (device, p, q, zeros, beta, designer mode).  No atomics: the saturation count of an int16 row
// is the sum of per-tile counts (workspace `ws`) taken by a second launch in a fixed order.
#include "segan_signal.h"

#define RS_THREADS 256
#define RS_TILE 256           // outputs per workgroup, one per thread
#define RS_CHUNK 2048         // input samples staged per pass (16 KiB of LDS)
#define RS_TAPS_LDS 2048      // tables up to this many doubles are staged in LDS
#define RS_RATE_MIN 4000
#define RS_RATE_MAX 192000
#define RS_ZEROS_MAX 64
#define RS_BETA_MAX 20.0
#define RS_MX_MAX 4096
#define RS_LY_MAX (1ll << 30)

#define RS_UNSUPPORTED(cond, ...)                \
  do {                                           \
    if (!(cond)) {                               \
      segan_set_error(__VA_ARGS__);              \
      return SEGAN_EUNSUPPORTED;                 \
    }                                            \
  } while (0)

namespace {

// -1 for arguments that are no rates / filter parameters at all, -3 for ones outside the limits
int rs_check(const char* what, int rate_in, int rate_out, int zeros, double beta, int* p, int* q) {
  SEGAN_REQUIRE(rate_in > 0 && rate_out > 0, "%s: bad rates %d -> %d Hz", what, rate_in, rate_out);
  SEGAN_REQUIRE(zeros > 0, "%s: bad zeros=%d", what, zeros);
  SEGAN_REQUIRE(beta >= 0.0 && beta < INFINITY, "%s: bad beta=%g", what, beta);
  RS_UNSUPPORTED(rate_in >= RS_RATE_MIN && rate_in <= RS_RATE_MAX && rate_out >= RS_RATE_MIN &&
                     rate_out <= RS_RATE_MAX,
                 "%s: rates %d -> %d Hz outside %d .. %d Hz", what, rate_in, rate_out, RS_RATE_MIN,
                 RS_RATE_MAX);
  RS_UNSUPPORTED(zeros <= RS_ZEROS_MAX, "%s: zeros=%d above %d", what, zeros, RS_ZEROS_MAX);
  RS_UNSUPPORTED(beta <= RS_BETA_MAX, "%s: beta=%g above %g", what, beta, RS_BETA_MAX);
  segan_reduce_ratio(rate_out, rate_in, p, q);
  RS_UNSUPPORTED(*p <= RS_MX_MAX && *q <= RS_MX_MAX,
                 "%s: %d -> %d Hz reduces to %d / %d, max(p, q) above %d", what, rate_in, rate_out,
                 *p, *q, RS_MX_MAX);
  return SEGAN_OK;
}

int rs_dims(const char* what, int T, int p, int q, int* Ly) {
  SEGAN_REQUIRE(T >= 0, "%s: bad length T=%d", what, T);
  const long long L = segan_resampled_len(T, p, q);
  RS_UNSUPPORTED(L <= RS_LY_MAX, "%s: T=%d converts to %lld samples (at most 2^30)", what, T, L);
  *Ly = (int)L;
  return SEGAN_OK;
}

struct ResampleTables {
  int device, p, q, zeros, lh, K;
  double beta;
  bool compensate;
  double* tab;   // [K][p], visiting order: tab[j p + s] = G[t_hi(s) - j p] (0 below -lh)
};

SeganDeviceTables<ResampleTables> g_rs_tables;

const ResampleTables* rs_get_tables(int p, int q, int zeros, double beta, bool compensate) {
  return g_rs_tables.get(
      "resample",
      [=](const ResampleTables& t) {
        return t.p == p && t.q == q && t.zeros == zeros && t.beta == beta &&
               t.compensate == compensate;
      },
      [=](ResampleTables* t) {
        std::vector<double> taps;
        segan_kaiser_sinc_taps(p, q, zeros, beta, compensate, &taps);
        const int lh = ((int)taps.size() - 1) / 2, K = 2 * lh / p + 1;
        t->p = p;
        t->q = q;
        t->zeros = zeros;
        t->beta = beta;
        t->compensate = compensate;
        t->lh = lh;
        t->K = K;
        std::vector<double> tab((size_t)K * p);
        for (int s = 0; s < p; ++s) {
          const int phi = (int)(((long long)s * q) % p);
          const int t_hi = phi + p * ((lh - phi) / p);   // the largest t <= lh with t = phi (mod p)
          for (int j = 0; j < K; ++j) {
            const int tt = t_hi - j * p;
            tab[(size_t)j * p + s] = tt >= -lh ? taps[tt + lh] : 0.0;
          }
        }
        return segan_upload(&t->tab, tab, "resample");
      });
}

}  // namespace

void segan_reduce_ratio(int num, int den, int* p, int* q) {
  int a = num, b = den;   // gcd
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  *p = num / a;
  *q = den / a;
}

static double bessel_i0(double x) {   // sum_k ((x/2)^k / k!)^2
  const double y = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200 && term > 1e-18 * sum; ++k) {
    term *= y / ((double)k * (double)k);
    sum += term;
  }
  return sum;
}

// numpy's sinc and kaiser expressions; p == q == 1 is the identity.  sum(h) is taken in index
// order, as the STOI oracle's np.sum over these few terms comes out and as STOI's fixtures pin
// it.  With `compensate` the taps are instead held to 1e-15 (absolute) of the exactly normalised
// filter: where the index order's rounding error alone moves the largest tap (p / sum(h), at
// h = 1) by more than RS_TAP_TOL — over thousands of terms it reaches 1e-14 of the sum — the
// compensated (Neumaier) sum, exact to the last bit or two, normalises.  Elsewhere the two modes
// give the same bits.
#define RS_TAP_TOL 1.0e-15

void segan_kaiser_sinc_taps(int p, int q, int zeros, double beta, bool compensate,
                            std::vector<double>* taps) {
  if (p == 1 && q == 1) {
    taps->assign(1, 1.0);
    return;
  }
  const int mx = p > q ? p : q;
  const int lh = zeros * mx, L = 2 * lh + 1;
  const double alpha = (L - 1) / 2.0, i0b = bessel_i0(beta);
  std::vector<double> h(L);
  double sum = 0.0;               // index order
  double ks = 0.0, kc = 0.0;      // Neumaier: ks + kc
  for (int n = 0; n < L; ++n) {
    const double u = (double)(n - lh) / (double)mx;
    const double y = M_PI * (u == 0.0 ? 1.0e-20 : u);
    const double r = (n - alpha) / alpha;
    h[n] = sin(y) / y * (bessel_i0(beta * sqrt(1.0 - r * r)) / i0b);
    sum += h[n];
    const double t = ks + h[n];
    kc += fabs(ks) >= fabs(h[n]) ? (ks - t) + h[n] : (h[n] - t) + ks;
    ks = t;
  }
  const double exact = ks + kc;
  if (compensate && fabs(p / sum - p / exact) > RS_TAP_TOL) sum = exact;
  taps->resize(L);
  for (int n = 0; n < L; ++n) (*taps)[n] = p * h[n] / sum;
}

__device__ __forceinline__ void rs_store(double* y, double v, bool* clipped) { *y = v; }
__device__ __forceinline__ void rs_store(float* y, double v, bool* clipped) { *y = (float)v; }
// round half to even, saturate (a NaN, possible only with a NaN fp32 input, becomes 0)
__device__ __forceinline__ void rs_store(int16_t* y, double v, bool* clipped) {
  double r = rint(v);
  if (!(r == r)) r = 0.0;
  *clipped = r > 32767.0 || r < -32768.0;
  r = r > 32767.0 ? 32767.0 : (r < -32768.0 ? -32768.0 : r);
  *y = (int16_t)(int)r;
}

// ---------------------------------------------------------------------------------
// y[r][m], m in the tile blockIdx.x of row blockIdx.y.  Thread t owns output m = tile RS_TILE + t:
// s = m mod p selects its column of the table, nf = (m q - t_hi) / p is the input sample its
// first tap meets (negative near the row's start), kphi the taps of its phase.  out_lengths[r]
// (optional) = the row's ceil(Lx p / q); tile_clip[r][tile] (int16 output, optional) = the
// tile's saturated samples.  Outputs from the row's length to Ly_max are zero.
// ---------------------------------------------------------------------------------
template <typename TI, typename TO, bool LDS_TAPS>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(
    const TI* __restrict__ x, const int* __restrict__ lengths, TO* __restrict__ y,
    int* __restrict__ out_lengths, int* __restrict__ tile_clip, int T, int Ly_max, int p, int q,
    int lh, int K, const double* __restrict__ tab) {
  __shared__ double xs[RS_CHUNK];
  __shared__ double tl[LDS_TAPS ? RS_TAPS_LDS : 1];
  __shared__ int wclip[RS_THREADS / 64];
  const int r = blockIdx.y, t = threadIdx.x;
  const int m0 = blockIdx.x * RS_TILE, m = m0 + t;
  const int Lx = segan_row_samples(lengths, r, T);
  const int Ly = (int)segan_resampled_len(Lx, p, q);
  if (blockIdx.x == 0 && t == 0 && out_lengths) out_lengths[r] = Ly;
  const double* tp = tab;
  if (LDS_TAPS) {
    for (int i = t; i < K * p; i += RS_THREADS) tl[i] = tab[i];   // the first barrier below orders it
    tp = tl;
  }
  double acc = 0.0;
  if (m0 < Ly) {   // the whole workgroup takes the same branch
    const TI* xrow = x + (size_t)r * T;
    const int mend = m0 + RS_TILE < Ly ? m0 + RS_TILE : Ly;
    // the input span of the tile's valid outputs m0 .. mend - 1
    const long long c0 = (long long)m0 * q, c1 = (long long)(mend - 1) * q;
    const long long nlo = c0 - lh <= 0 ? 0 : (c0 - lh + p - 1) / p;
    long long nhi = (c1 + lh) / p;
    nhi = nhi < Lx - 1 ? nhi : Lx - 1;
    // this thread's taps j = jlo .. jhi meet the samples nf + j
    const bool active = m < Ly;
    const long long c = (long long)m * q;
    const int s = m % p, phi = (int)(c % p);
    const int t_hi = phi + p * ((lh - phi) / p);
    const long long nf = (c - t_hi) / p;   // exact: c - t_hi is a multiple of p
    const int kphi = (t_hi + lh) / p + 1;
    const long long jlo = nf < 0 ? -nf : 0;
    const long long jhi = kphi - 1 < Lx - 1 - nf ? kphi - 1 : Lx - 1 - nf;
    for (long long a = nlo; a <= nhi; a += RS_CHUNK) {
      const int cnt = nhi - a + 1 < RS_CHUNK ? (int)(nhi - a + 1) : RS_CHUNK;
      __syncthreads();   // the previous pass has been read
      for (int i = t; i < cnt; i += RS_THREADS) xs[i] = (double)xrow[a + i];
      __syncthreads();
      if (active) {
        const long long ja = jlo > a - nf ? jlo : a - nf;
        const long long jb = jhi < a + cnt - 1 - nf ? jhi : a + cnt - 1 - nf;
        const int off = (int)(nf - a);   // sample nf + j sits at xs[off + j]
        for (int j = (int)ja; j <= (int)jb; ++j) acc = fma(xs[off + j], tp[j * p + s], acc);
      }
    }
  }
  bool clipped = false;
  if (m < Ly_max) rs_store(y + (size_t)r * Ly_max + m, acc, &clipped);
  if (tile_clip) {   // int16 output only
    const unsigned long long b = __ballot(clipped);
    if ((t & 63) == 0) wclip[t >> 6] = __popcll(b);
    __syncthreads();
    if (t == 0)
      tile_clip[(size_t)r * gridDim.x + blockIdx.x] = wclip[0] + wclip[1] + wclip[2] + wclip[3];
  }
}

// nclip[r] = the sum of the row's tile counts, one wave per row
__global__ __launch_bounds__(RS_THREADS) void resample_nclip_kernel(
    const int* __restrict__ tile_clip, int* __restrict__ nclip, int rows, int tiles) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (RS_THREADS / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;   // whole waves leave
  const int* row = tile_clip + (size_t)r * tiles;
  int s = 0;
  for (int k = lane; k < tiles; k += 64) s += row[k];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) nclip[r] = s;
}

namespace {

template <typename TI, typename TO>
void rs_launch(const void* x, const int* lengths, void* y, int* out_lengths, int* tile_clip,
               int rows, int T, int Ly_max, const ResampleTables* tb, hipStream_t st) {
  const dim3 grid(ceil_div(Ly_max, RS_TILE), rows), blk(RS_THREADS);
  if ((long long)tb->K * tb->p <= RS_TAPS_LDS)
    hipLaunchKernelGGL((resample_kernel<TI, TO, true>), grid, blk, 0, st, (const TI*)x, lengths,
                       (TO*)y, out_lengths, tile_clip, T, Ly_max, tb->p, tb->q, tb->lh, tb->K,
                       tb->tab);
  else
    hipLaunchKernelGGL((resample_kernel<TI, TO, false>), grid, blk, 0, st, (const TI*)x, lengths,
                       (TO*)y, out_lengths, tile_clip, T, Ly_max, tb->p, tb->q, tb->lh, tb->K,
                       tb->tab);
}

template <typename TI>
void rs_launch_out(int y_dtype, const void* x, const int* lengths, void* y, int* out_lengths,
                   int* tile_clip, int rows, int T, int Ly_max, const ResampleTables* tb,
                   hipStream_t st) {
  if (y_dtype == SEGAN_DT_F64)
    rs_launch<TI, double>(x, lengths, y, out_lengths, nullptr, rows, T, Ly_max, tb, st);
  else if (y_dtype == SEGAN_DT_F32)
    rs_launch<TI, float>(x, lengths, y, out_lengths, nullptr, rows, T, Ly_max, tb, st);
  else
    rs_launch<TI, int16_t>(x, lengths, y, out_lengths, tile_clip, rows, T, Ly_max, tb, st);
}

}  // namespace

int segan_resample_rows(int p, int q, int zeros, double beta, bool compensate, const void* x,
                        int x_dtype, const int* lengths, int rows, int T, void* y, int y_dtype,
                        int Ly_max, int* out_lengths, int* tile_clip, hipStream_t stream) {
  const ResampleTables* tb = rs_get_tables(p, q, zeros, beta, compensate);
  if (!tb) return SEGAN_ELAUNCH;
  if (x_dtype == SEGAN_DT_F32)
    rs_launch_out<float>(y_dtype, x, lengths, y, out_lengths, tile_clip, rows, T, Ly_max, tb,
                         stream);
  else
    rs_launch_out<int16_t>(y_dtype, x, lengths, y, out_lengths, tile_clip, rows, T, Ly_max, tb,
                           stream);
  return SEGAN_OK;
}

extern "C" int segan_resample_plan(int rate_in, int rate_out, int zeros, double beta, int* pq,
                                   int* ntaps, double* taps, int cap) {
  SEGAN_REQUIRE(pq && ntaps, "resample_plan: NULL pointer");
  int p, q;
  if (int e = rs_check("resample_plan", rate_in, rate_out, zeros, beta, &p, &q)) return e;
  pq[0] = p;
  pq[1] = q;
  *ntaps = (p == 1 && q == 1) ? 1 : 2 * zeros * (p > q ? p : q) + 1;
  if (taps) {
    SEGAN_REQUIRE(cap >= *ntaps, "resample_plan: %d taps do not fit in %d", *ntaps, cap);
    std::vector<double> g;
    segan_kaiser_sinc_taps(p, q, zeros, beta, true, &g);
    for (int n = 0; n < *ntaps; ++n) taps[n] = g[n];
  }
  return SEGAN_OK;
}

extern "C" int segan_resample_dims(int T, int rate_in, int rate_out, int* dims) {
  SEGAN_REQUIRE(dims, "resample_dims: NULL pointer");
  int p, q, Ly;
  if (int e = rs_check("resample_dims", rate_in, rate_out, 1, 0.0, &p, &q)) return e;
  if (int e = rs_dims("resample_dims", T, p, q, &Ly)) return e;
  dims[0] = Ly;
  dims[1] = RS_TILE;
  return SEGAN_OK;
}

extern "C" int segan_resample(const void* x, int x_dtype, const int* lengths, int rows, int T,
                              int rate_in, int rate_out, int zeros, double beta, void* y,
                              int y_dtype, int Ly_max, int* out_lengths, int* nclip, int* ws,
                              void* stream) {
  SEGAN_REQUIRE(x && y, "resample: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && T > 0, "resample: bad sizes rows=%d T=%d", rows, T);
  SEGAN_REQUIRE(x_dtype == SEGAN_DT_F32 || x_dtype == SEGAN_DT_I16,
                "resample: x_dtype %d is neither fp32 nor int16", x_dtype);
  SEGAN_REQUIRE(y_dtype == SEGAN_DT_F32 || y_dtype == SEGAN_DT_I16 || y_dtype == SEGAN_DT_F64,
                "resample: y_dtype %d is none of fp32, int16, fp64", y_dtype);
  int p, q, Ly;
  if (int e = rs_check("resample", rate_in, rate_out, zeros, beta, &p, &q)) return e;
  if (int e = rs_dims("resample", T, p, q, &Ly)) return e;
  SEGAN_REQUIRE(Ly_max >= Ly, "resample: Ly_max=%d below the %d samples T=%d converts to", Ly_max,
                Ly, T);
  RS_UNSUPPORTED(Ly_max <= RS_LY_MAX, "resample: Ly_max=%d above 2^30", Ly_max);
  const bool count = y_dtype == SEGAN_DT_I16 && nclip;
  SEGAN_REQUIRE(!count || ws, "resample: int16 output with nclip needs the workspace ws");
  hipStream_t st = (hipStream_t)stream;
  if (int e = segan_resample_rows(p, q, zeros, beta, true, x, x_dtype, lengths, rows, T, y, y_dtype,
                                  Ly_max, out_lengths, count ? ws : nullptr, st))
    return e;
  if (count)
    hipLaunchKernelGGL(resample_nclip_kernel, dim3(ceil_div(rows, RS_THREADS / 64)),
                       dim3(RS_THREADS), 0, st, ws, nclip, rows, ceil_div(Ly_max, RS_TILE));
  else if (nclip && hipMemsetAsync(nclip, 0, (size_t)rows * sizeof(int), st) != hipSuccess) {
    segan_set_error("resample: clearing nclip failed");
    return SEGAN_ELAUNCH;
  }
  return segan_check_launch("resample");
}
