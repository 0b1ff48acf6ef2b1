// segan_distort.hip — on-the-fly signal-level distortions (the numpy oracle
// is scripts/distort_oracle.py):
//   * segan_clip_rows: amplitude clipping at a fraction of the row's own peak;
//   * segan_chop_rows: up to 8 chunks per row zeroed where the P.56 envelope says there is speech;
//   * segan_fir_rows: a zero-phase (symmetric) low-pass FIR per row, chosen from a bank.
// One workgroup per row (per tile of a row for the FIR), no atomics, no scratch: every count and
// sum runs in an order that depends only on the row's own data, so a row's result depends on
// neither the other rows nor its position in the batch.  Products and sums round on their own
// (no contraction into fma).
#include "segan_signal.h"

#pragma clang fp contract(off)

#define DS_THREADS 256
#define DS_WAVES (DS_THREADS / 64)
#define DS_E 4                                  // ballots per wave and slab of the chop
#define DS_SLAB (DS_THREADS * DS_E)             // samples per slab
#define DS_TILE SEGAN_FIR_TILE                  // outputs per workgroup of the FIR
#define DS_OUT (DS_TILE / DS_THREADS)           // outputs per thread
#define DS_KMAX SEGAN_FIR_MAX_K

static_assert(DS_TILE % DS_THREADS == 0, "whole outputs per thread");
static_assert((DS_TILE + 2 * DS_KMAX) * 4 + (DS_KMAX + 1) * 8 <= 64 * 1024, "LDS of the FIR");

namespace {

// sum of an int over the workgroup; every thread gets it.  `sh` holds DS_WAVES ints.
__device__ __forceinline__ int ds_block_sum(int v, int* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // sh of an earlier call has been read
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < DS_WAVES; ++w) s += sh[w];
  return s;
}

// position of the k-th set bit (from 0) of m; k < popcount(m)
__device__ __forceinline__ int ds_select64(unsigned long long m, int k) {
  int pos = 0;
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) {
    const int c = __popcll((m >> pos) & ((1ull << w) - 1ull));
    if (k >= c) {
      k -= c;
      pos += w;
    }
  }
  return pos;
}

}  // namespace

// ---------------------------------------------------------------------------------
// Clip.  m = max |x[:len]| (a max of fp32 values: exact in any order), thr = (float)(factor m)
// with the product in double, y = min(max(x, -thr), thr); prev is clamped the same way.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void clip_rows_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const float* __restrict__ prev,
    const double* __restrict__ factor, float* __restrict__ y, float* __restrict__ prev_out,
    float* __restrict__ mout, float* __restrict__ throut, int* __restrict__ nclipped,
    int* __restrict__ status, int T) {
  __shared__ float wmax[DS_WAVES];
  __shared__ int wsum[DS_WAVES];
  const int r = blockIdx.x, t = threadIdx.x;
  const int L = segan_row_samples(lengths, r, T);
  const float* xr = x + (size_t)r * T;
  float* yr = y + (size_t)r * T;

  float m = 0.0f;
  for (int i = t; i < L; i += DS_THREADS) m = fmaxf(m, fabsf(xr[i]));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  if ((t & 63) == 0) wmax[t >> 6] = m;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < DS_WAVES; ++w) m = fmaxf(m, wmax[w]);

  const double f = factor[r];
  int st = 0;
  if (L == 0 || m == 0.0f) st |= SEGAN_CLIP_ST_SILENT;
  if (!(f > 0.0 && f <= 1.0)) st |= SEGAN_CLIP_ST_FACTOR;
  const float thr = (st & SEGAN_CLIP_ST_FACTOR) ? 0.0f : (float)(f * (double)m);
  int changed = 0;
  for (int i = t; i < T; i += DS_THREADS) {
    const float v = xr[i];
    float o = v;
    if (!st && i < L) o = fminf(fmaxf(v, -thr), thr);
    changed += o != v ? 1 : 0;
    yr[i] = o;
  }
  changed = ds_block_sum(changed, wsum);
  if (t == 0) {
    if (prev_out) {
      const float p = prev[r];
      prev_out[r] = st ? p : fminf(fmaxf(p, -thr), thr);
    }
    mout[r] = m;
    throut[r] = thr;
    nclipped[r] = changed;
    status[r] = st;
  }
}

// ---------------------------------------------------------------------------------
// Chop.  Sample t < len is active when q[t] >= c0.  A row is walked in slabs of DS_SLAB samples:
// wave w of a slab takes DS_E ballots of 64 consecutive samples each, in index order.
//   pass 1: n = the number of active samples (popcounts; integers, so any order gives n);
//   pass 2: the count before each wave's samples is carried from slab to slab; the wave whose
//           samples hold the k_c-th active one finds it by a rank select on its ballots;
//   pass 3: y = 0 inside the union of [start_c, min(start_c + dur_c, len)), x elsewhere.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(DS_THREADS) void chop_rows_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const double* __restrict__ q,
    const double* __restrict__ c0, const double* __restrict__ u, const int* __restrict__ dur,
    float* __restrict__ y, int* __restrict__ starts, int* __restrict__ nactive,
    int* __restrict__ nzeroed, int* __restrict__ status, int T, int C) {
  __shared__ int wcnt[DS_WAVES];
  __shared__ int wsum[DS_WAVES];
  __shared__ int tk[SEGAN_CHOP_MAX], tstart[SEGAN_CHOP_MAX];
  __shared__ long long tend[SEGAN_CHOP_MAX];
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int L = segan_row_samples(lengths, r, T);
  const float* xr = x + (size_t)r * T;
  const double* qr = q + (size_t)r * T;
  float* yr = y + (size_t)r * T;
  const double thr = c0[r];   // NaN: no comparison holds, nothing is active

  int mine = 0;   // the active samples this wave has seen (the same in all its lanes)
  for (int base = 0; base < L; base += DS_SLAB) {
#pragma unroll
    for (int e = 0; e < DS_E; ++e) {
      const int i = base + (wave * DS_E + e) * 64 + lane;
      mine += __popcll(__ballot(i < L && qr[i] >= thr));
    }
  }
  if (lane == 0) wcnt[wave] = mine;
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int w = 0; w < DS_WAVES; ++w) n += wcnt[w];

  if (t < SEGAN_CHOP_MAX) {
    int k = -1;
    if (t < C && n > 0 && dur[(size_t)r * C + t] > 0) {
      const double uc = u[(size_t)r * C + t];
      const double pos = floor(uc * (double)n);
      k = !(pos >= 0.0) ? 0 : (pos >= (double)n ? n - 1 : (int)(long long)pos);
    }
    tk[t] = k;
    tstart[t] = -1;
  }
  __syncthreads();   // also: wcnt has been read

  int carry = 0;   // active samples before this slab
  for (int base = 0; n > 0 && base < L; base += DS_SLAB) {
    unsigned long long b[DS_E];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < DS_E; ++e) {
      const int i = base + (wave * DS_E + e) * 64 + lane;
      b[e] = __ballot(i < L && qr[i] >= thr);
      cnt += __popcll(b[e]);
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    int before = carry, total = carry;
#pragma unroll
    for (int w = 0; w < DS_WAVES; ++w) {
      if (w < wave) before += wcnt[w];
      total += wcnt[w];
    }
    for (int c = 0; c < C; ++c) {
      int k = tk[c] - before;   // uniform over the wave
      if (tk[c] < 0 || k < 0 || k >= cnt) continue;
#pragma unroll
      for (int e = 0; e < DS_E; ++e) {
        const int pc = __popcll(b[e]);
        if (k >= 0 && k < pc) {
          if (lane == 0) tstart[c] = base + (wave * DS_E + e) * 64 + ds_select64(b[e], k);
          k = -1;
        } else if (k >= 0) {
          k -= pc;
        }
      }
    }
    carry = total;
    __syncthreads();   // wcnt has been read
  }
  __syncthreads();
  if (t < SEGAN_CHOP_MAX) {
    long long end = -1;
    if (tstart[t] >= 0) {
      end = (long long)tstart[t] + (long long)dur[(size_t)r * C + t];
      if (end > L) end = L;
    }
    tend[t] = end;
    if (t < C) starts[(size_t)r * C + t] = tstart[t];
  }
  __syncthreads();

  int s0[SEGAN_CHOP_MAX];
  long long s1[SEGAN_CHOP_MAX];
#pragma unroll
  for (int c = 0; c < SEGAN_CHOP_MAX; ++c) {
    s0[c] = tstart[c];
    s1[c] = tend[c];
  }
  int zeroed = 0;
  for (int i = t; i < T; i += DS_THREADS) {
    bool z = false;
#pragma unroll
    for (int c = 0; c < SEGAN_CHOP_MAX; ++c) z = z || (s0[c] >= 0 && i >= s0[c] && i < s1[c]);
    zeroed += z ? 1 : 0;
    yr[i] = z ? 0.0f : xr[i];
  }
  zeroed = ds_block_sum(zeroed, wsum);
  if (t == 0) {
    nactive[r] = n;
    nzeroed[r] = zeroed;
    status[r] = n == 0 ? SEGAN_CHOP_ST_NOLEVEL : 0;
  }
}

// ---------------------------------------------------------------------------------
// FIR.  Output index j = n + 1, n = -1 .. T-1 (j = 0 is prev_out); workgroup (tile, row) computes
// outputs j0 .. j0 + DS_TILE - 1 from xe[n0 - K .. n0 + DS_TILE - 1 + K] and the row's taps, both
// staged in LDS.  Thread t owns outputs j0 + t + 256 i: neighbouring lanes read neighbouring
// words, and one tap read from LDS serves DS_OUT accumulators held in registers.
//   y[n] = h[0] xe[n] + sum_{k = 1 .. K} h[k] (xe[n-k] + xe[n+k]),  k ascending, fp64
// The order is per output and does not involve the tile.
// ---------------------------------------------------------------------------------
template <typename TY>
__global__ __launch_bounds__(DS_THREADS) void fir_rows_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const float* __restrict__ prev,
    const double* __restrict__ bank, const int* __restrict__ Ks, int nf, int kmax,
    const int* __restrict__ ids, TY* __restrict__ y, TY* __restrict__ prev_out,
    int* __restrict__ status, int T) {
  __shared__ float xs[DS_TILE + 2 * DS_KMAX];
  __shared__ double hs[DS_KMAX + 1];
  const int r = blockIdx.y, t = threadIdx.x;
  const int j0 = blockIdx.x * DS_TILE, n0 = j0 - 1;
  const int L = segan_row_samples(lengths, r, T);
  const float* xr = x + (size_t)r * T;
  TY* yr = y + (size_t)r * T;
  const float pv = prev ? prev[r] : 0.0f;
  const int id = ids[r];
  int K = -1;
  if (id >= 0 && id < nf) K = Ks[id];
  const bool bad = K < 0 || K > kmax;
  if (blockIdx.x == 0 && t == 0) status[r] = bad ? SEGAN_FIR_ST_ID : 0;

  if (bad || n0 >= L) {   // a flagged row is copied; a tile past the row's length is zero
    for (int i = t; i < DS_TILE; i += DS_THREADS) {
      const int j = j0 + i;
      if (j > T) break;
      if (j == 0)
        prev_out[r] = (TY)pv;   // reached with a flagged row only (n0 = -1 < L otherwise)
      else
        yr[j - 1] = bad ? (TY)xr[j - 1] : (TY)0;
    }
    return;
  }

  const double* h = bank + (size_t)id * (kmax + 1);
  for (int k = t; k <= K; k += DS_THREADS) hs[k] = h[k];
  for (int e = t; e < DS_TILE + 2 * K; e += DS_THREADS) {
    const int n = n0 - K + e;
    xs[e] = n == -1 ? pv : (n >= 0 && n < L ? xr[n] : 0.0f);
  }
  __syncthreads();

  double acc[DS_OUT];
  const double h0 = hs[0];
#pragma unroll
  for (int i = 0; i < DS_OUT; ++i) acc[i] = h0 * (double)xs[K + t + DS_THREADS * i];
  for (int k = 1; k <= K; ++k) {
    const double hk = hs[k];
#pragma unroll
    for (int i = 0; i < DS_OUT; ++i) {
      const int c = K + t + DS_THREADS * i;
      const double s = (double)xs[c - k] + (double)xs[c + k];
      const double p = hk * s;
      acc[i] = acc[i] + p;
    }
  }
#pragma unroll
  for (int i = 0; i < DS_OUT; ++i) {
    const int j = j0 + t + DS_THREADS * i;
    if (j > T) continue;
    if (j == 0)
      prev_out[r] = (TY)acc[i];
    else
      yr[j - 1] = j - 1 < L ? (TY)acc[i] : (TY)0;
  }
}

static int ds_rows_ok(const char* what, int rows, int T) {
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && T > 0 && (long long)T <= (1ll << 30),
                "%s: bad sizes rows=%d T=%d", what, rows, T);
  return SEGAN_OK;
}

extern "C" int segan_clip_rows(const float* x, const int* lengths, const float* prev,
                               const double* factor, int rows, int T, float* y, float* prev_out,
                               float* m, float* thr, int* nclipped, int* status, void* stream) {
  SEGAN_REQUIRE(x && factor && y && m && thr && nclipped && status, "clip_rows: NULL pointer");
  SEGAN_REQUIRE((prev == nullptr) == (prev_out == nullptr),
                "clip_rows: prev and prev_out go together");
  if (int e = ds_rows_ok("clip_rows", rows, T)) return e;
  hipLaunchKernelGGL(clip_rows_kernel, dim3(rows), dim3(DS_THREADS), 0, (hipStream_t)stream, x,
                     lengths, prev, factor, y, prev_out, m, thr, nclipped, status, T);
  return segan_check_launch("clip_rows_kernel");
}

extern "C" int segan_chop_rows(const float* x, const int* lengths, const double* q,
                               const double* c0, const double* u, const int* dur, int rows, int T,
                               int C, float* y, int* starts, int* nactive, int* nzeroed,
                               int* status, void* stream) {
  SEGAN_REQUIRE(x && q && c0 && u && dur && y && starts && nactive && nzeroed && status,
                "chop_rows: NULL pointer");
  if (int e = ds_rows_ok("chop_rows", rows, T)) return e;
  SEGAN_REQUIRE(C >= 1 && C <= SEGAN_CHOP_MAX, "chop_rows: 1 .. %d chunks per row, got %d",
                SEGAN_CHOP_MAX, C);
  hipLaunchKernelGGL(chop_rows_kernel, dim3(rows), dim3(DS_THREADS), 0, (hipStream_t)stream, x,
                     lengths, q, c0, u, dur, y, starts, nactive, nzeroed, status, T, C);
  return segan_check_launch("chop_rows_kernel");
}

extern "C" int segan_fir_rows(const float* x, const int* lengths, const float* prev,
                              const double* bank, const int* K, int nf, int kmax, const int* ids,
                              int rows, int T, void* y, int y_dtype, void* prev_out, int* status,
                              void* stream) {
  SEGAN_REQUIRE(x && bank && K && ids && y && prev_out && status, "fir_rows: NULL pointer");
  if (int e = ds_rows_ok("fir_rows", rows, T)) return e;
  SEGAN_REQUIRE(nf > 0 && kmax >= 0 && kmax <= SEGAN_FIR_MAX_K,
                "fir_rows: bad bank nf=%d kmax=%d (kmax <= %d)", nf, kmax, SEGAN_FIR_MAX_K);
  SEGAN_REQUIRE(y_dtype == SEGAN_DT_F32 || y_dtype == SEGAN_DT_F64,
                "fir_rows: y_dtype %d is neither fp32 nor fp64", y_dtype);
  const dim3 grid(ceil_div(T + 1, DS_TILE), rows);
  if (y_dtype == SEGAN_DT_F64)
    hipLaunchKernelGGL(fir_rows_kernel<double>, grid, dim3(DS_THREADS), 0, (hipStream_t)stream, x,
                       lengths, prev, bank, K, nf, kmax, ids, (double*)y, (double*)prev_out,
                       status, T);
  else
    hipLaunchKernelGGL(fir_rows_kernel<float>, grid, dim3(DS_THREADS), 0, (hipStream_t)stream, x,
                       lengths, prev, bank, K, nf, kmax, ids, (float*)y, (float*)prev_out, status,
                       T);
  return segan_check_launch("fir_rows_kernel");
}
