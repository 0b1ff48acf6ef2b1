// BSS-eval signal-to-distortion ratio with a distortion filter of up to 512 taps (the SDR of
// bss_eval_sources): the processed row x is projected onto the span of the
// clean row s and its first taps - 1 delays, and the ratio is taken between that projection and the
// rest.  fp64 on fp32 rows, per-row lengths, no atomics, every sum in an order fixed by the sample
// index alone, so a row's result depends neither on T, nor on the other rows, nor on what lies
// past its length, and two calls return the same bits.
//
//   sdr_corr_kernel    one workgroup per (span of SEGAN_SDR_SPAN samples, row): the span's share of
//                      r[k] = sum s[t] s[t+k] and d[k] = sum s[t] x[t+k], k < taps
//   sdr_corr_sum_kernel  the spans added in ascending order
//   toeplitz_solve_kernel  Toeplitz(r) c = d by the Levinson recursion, one wave per row
//   sdr_fir_kernel     one workgroup per (span, row) of t in [0, L + taps - 1): st = c * s and the
//                      span's share of St = sum st^2, Ee = sum (x - st)^2
//   sdr_final_kernel   one wave per row: the spans added, the value and its special cases
#include "segan_signal.h"

#define SDR_THREADS 256
#define SDR_LANE_TAPS (SEGAN_SDR_MAX_TAPS / 64)   // taps a lane of the solver holds
#define SDR_ROWS_PER_WG (SDR_THREADS / 64)        // the solver's rows per workgroup
#define SDR_T_PER_THREAD (SEGAN_SDR_SPAN / SDR_THREADS)
#define SDR_GUARD 0x1p-40                         // the recursion stops at E_m <= SDR_GUARD r[0]

static_assert(SEGAN_SDR_MAX_TAPS == 2 * SDR_THREADS, "sdr_corr_kernel: two lags per thread");
static_assert(SEGAN_SDR_SPAN % (2 * SDR_THREADS) == 0, "sdr_fir_kernel: whole strides of pairs");
static_assert(SEGAN_SDR_SPAN % 4 == 0, "sdr_corr_kernel: four samples at a time");

namespace {

// the doubles of one row's stage block: r[n], d[n], c[n], order, St, Ee
__host__ __device__ inline size_t sdr_stage_stride(int n) { return 3 * (size_t)n + 3; }

__host__ __device__ inline int sdr_spans(long long len) {
  return (int)((len + SEGAN_SDR_SPAN - 1) / SEGAN_SDR_SPAN);
}

// doubles of each of sdr_corr_kernel's two LDS arrays: the span, the n - 1 samples after it and
// what the last window of four samples reads past them, even (the second array stays 16-byte
// aligned)
__host__ __device__ inline int sdr_corr_ext(int n) { return (SEGAN_SDR_SPAN + n + 5) & ~1; }

// Lagged correlations of one span.  LDS holds s and x of [start, start + sdr_corr_ext(n)) as
// doubles, zero from the row's length on; thread t owns the lags 2t and 2t + 1 and walks the
// span's samples in ascending order, four at a time: s[t .. t+3] is a broadcast, the windows
// s / x[t + 2l .. t + 2l + 4] are two aligned 16-byte reads and one of 8 bytes, consecutive across
// lanes: 8 LDS reads per 16 FMAs.  r and d run through the same loop, and every product of two
// fp32 values is exact in fp64.  A last group of fewer than four samples is filled with the
// zeros past the row's length: they add exact zeros.
__global__ __launch_bounds__(SDR_THREADS) void sdr_corr_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, const int* __restrict__ lengths,
    int T, int n, int nspans, double* __restrict__ part) {
  extern __shared__ double2 sdr_sh[];
  const int r = blockIdx.y, tid = threadIdx.x;
  const int L = segan_row_samples(lengths, r, T);
  const long long start = (long long)blockIdx.x * SEGAN_SDR_SPAN;
  if (start >= L) return;   // the whole workgroup, before any barrier
  const int ext = sdr_corr_ext(n);
  double* sE = reinterpret_cast<double*>(sdr_sh);   // [ext]
  double* xE = sE + ext;                            // [ext]
  const float* s = ref + (size_t)r * T;
  const float* x = deg + (size_t)r * T;
  for (int i = tid; i < ext; i += SDR_THREADS) {
    const long long g = start + i;
    const bool in = g < L;
    sE[i] = in ? (double)s[g] : 0.0;
    xE[i] = in ? (double)x[g] : 0.0;
  }
  __syncthreads();
  if (2 * (tid & ~63) >= n) return;   // whole waves without a lag below n; no barrier below
  const int count = (int)(L - start < SEGAN_SDR_SPAN ? L - start : SEGAN_SDR_SPAN);
  const int k = 2 * tid < n ? 2 * tid : 0;   // lanes past n read lag 0's window and store nothing
  const double2* sa = reinterpret_cast<const double2*>(sE);
  const double2* sw = reinterpret_cast<const double2*>(sE + k);
  const double2* xw = reinterpret_cast<const double2*>(xE + k);
  double r0 = 0.0, d0 = 0.0, r1 = 0.0, d1 = 0.0;
  for (int t = 0; t < count; t += 4) {
    const int h = t >> 1;
    const double2 a01 = sa[h], a23 = sa[h + 1];
    const double2 s01 = sw[h], s23 = sw[h + 1];
    const double2 x01 = xw[h], x23 = xw[h + 1];
    const double s4 = sE[k + t + 4], x4 = xE[k + t + 4];
    r0 = fma(a01.x, s01.x, r0);
    d0 = fma(a01.x, x01.x, d0);
    r1 = fma(a01.x, s01.y, r1);
    d1 = fma(a01.x, x01.y, d1);
    r0 = fma(a01.y, s01.y, r0);
    d0 = fma(a01.y, x01.y, d0);
    r1 = fma(a01.y, s23.x, r1);
    d1 = fma(a01.y, x23.x, d1);
    r0 = fma(a23.x, s23.x, r0);
    d0 = fma(a23.x, x23.x, d0);
    r1 = fma(a23.x, s23.y, r1);
    d1 = fma(a23.x, x23.y, d1);
    r0 = fma(a23.y, s23.y, r0);
    d0 = fma(a23.y, x23.y, d0);
    r1 = fma(a23.y, s4, r1);
    d1 = fma(a23.y, x4, d1);
  }
  double* p = part + ((size_t)r * nspans + blockIdx.x) * 2 * (size_t)n;
  if (2 * tid < n) {
    p[2 * tid] = r0;
    p[n + 2 * tid] = d0;
  }
  if (2 * tid + 1 < n) {
    p[2 * tid + 1] = r1;
    p[n + 2 * tid + 1] = d1;
  }
}

// stage[row][0 .. 2n) = (r, d): the row's own spans added in ascending order, one thread per lag
__global__ __launch_bounds__(SDR_THREADS) void sdr_corr_sum_kernel(
    const int* __restrict__ lengths, int T, int n, int nspans, const double* __restrict__ part,
    double* __restrict__ stage) {
  const int r = blockIdx.y, k = blockIdx.x * SDR_THREADS + threadIdx.x;
  if (k >= 2 * n) return;
  int mine = sdr_spans(segan_row_samples(lengths, r, T));
  if (mine > nspans) mine = nspans;
  const double* p = part + (size_t)r * nspans * 2 * (size_t)n + k;
  double acc = 0.0;
  for (int b = 0; b < mine; ++b) acc += p[(size_t)b * 2 * n];
  stage[(size_t)r * sdr_stage_stride(n) + k] = acc;
}

// The writes of some lanes are read by others of the same wave: the wave runs in lockstep and
// its LDS accesses complete in order; this keeps the compiler from moving them across.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Toeplitz(r) c = d, r / d / c of n <= 512 doubles, by the Levinson recursion for a general
// right-hand side.  One wave per row, SDR_ROWS_PER_WG rows per workgroup, no workgroup barrier.
// Lane l holds a[j] (the predictor, a[0] = 0 here) and c[j] for j = l + 64 i in registers; r, d
// and a copy of a live in the wave's own LDS, where the reversed reads r[m - j], a[m - j] go.
// Step m: both dot products sum_j a[j] r[m-j] and sum_j c[j] r[m-j] (each lane its j ascending,
// then the butterfly: the same bits in every lane), k = -(r[m] + .) / E, a[j] += k a[m-j],
// a[m] = k, E *= 1 - k^2; if E <= 2^-40 r[0] the recursion stops with order m and c[m ..] = 0;
// else lambda = (d[m] - .) / E, c[j] += lambda a[m-j], c[m] = lambda.
__global__ __launch_bounds__(SDR_THREADS) void toeplitz_solve_kernel(
    const double* __restrict__ rg, const double* __restrict__ dg, size_t in_stride,
    double* __restrict__ cg, size_t c_stride, int* __restrict__ order_i,
    double* __restrict__ order_d, size_t order_stride, int rows, int n) {
  __shared__ double lds[SDR_ROWS_PER_WG][3][SEGAN_SDR_MAX_TAPS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * SDR_ROWS_PER_WG + wave;
  if (row >= rows) return;   // whole waves
  double* rl = lds[wave][0];
  double* dl = lds[wave][1];
  double* al = lds[wave][2];
  for (int j = lane; j < n; j += 64) {
    rl[j] = rg[(size_t)row * in_stride + j];
    dl[j] = dg[(size_t)row * in_stride + j];
    al[j] = 0.0;
  }
  wave_lds_fence();

  double a[SDR_LANE_TAPS], c[SDR_LANE_TAPS];
#pragma unroll
  for (int i = 0; i < SDR_LANE_TAPS; ++i) a[i] = c[i] = 0.0;
  const double r0 = rl[0], floor_e = SDR_GUARD * r0;
  double E = r0;
  int order = 0;
  for (int m = 0; m < n; ++m) {
    double sa = 0.0, sc = 0.0;
#pragma unroll
    for (int i = 0; i < SDR_LANE_TAPS; ++i) {
      const int j = lane + 64 * i;
      if (64 * i < m && j < m) {
        const double rr = rl[m - j];
        sa = fma(a[i], rr, sa);
        sc = fma(c[i], rr, sc);
      }
    }
    sa = segan_wave_sum(sa);
    sc = segan_wave_sum(sc);
    if (m > 0) {
      const double k = -(rl[m] + sa) / E;
      double rev[SDR_LANE_TAPS];
#pragma unroll
      for (int i = 0; i < SDR_LANE_TAPS; ++i) {
        const int j = lane + 64 * i;
        rev[i] = (64 * i < m && j >= 1 && j < m) ? al[m - j] : 0.0;
      }
      wave_lds_fence();   // every old a[m - j] is read before any a[j] is replaced
#pragma unroll
      for (int i = 0; i < SDR_LANE_TAPS; ++i) {
        const int j = lane + 64 * i;
        if (64 * i <= m) {
          if (j >= 1 && j < m) a[i] = fma(k, rev[i], a[i]);
          if (j == m) a[i] = k;
          if (j >= 1 && j <= m) al[j] = a[i];
        }
      }
      wave_lds_fence();
      E = E * (1.0 - k * k);
    }
    if (!(E > floor_e)) break;   // the same bits in every lane: the whole wave leaves
    const double lambda = (dl[m] - sc) / E;
#pragma unroll
    for (int i = 0; i < SDR_LANE_TAPS; ++i) {
      const int j = lane + 64 * i;
      if (64 * i <= m) {
        if (j < m) c[i] = fma(lambda, al[m - j], c[i]);
        if (j == m) c[i] = lambda;
      }
    }
    order = m + 1;
  }
#pragma unroll
  for (int i = 0; i < SDR_LANE_TAPS; ++i) {
    const int j = lane + 64 * i;
    if (j < n) cg[(size_t)row * c_stride + j] = j < order ? c[i] : 0.0;
  }
  if (lane == 0) {
    if (order_i) order_i[row] = order;
    if (order_d) order_d[(size_t)row * order_stride] = (double)order;
  }
}

// st[t] = sum_k c[k] s[t - k] (k ascending) for the span's t in [start, start + SPAN) below
// L + n - 1, and the span's (sum st^2, sum (x - st)^2).  LDS holds s of [start - P, start + SPAN)
// as doubles (P = n rounded up to even; zero outside [0, L)) and c, zero from n on; thread t owns
// the sample pairs 2t + 512 i, 2t + 512 i + 1 and takes the taps two at a time: (c[k], c[k+1])
// is a broadcast, (s[t-k], s[t-k+1]) one aligned 16-byte read and s[t-k-1] one of 8 bytes,
// consecutive across lanes: 2 LDS reads per 4 FMAs.  For an odd n the tap c[n] = 0 adds exact
// zeros.  Each thread sums its own samples in ascending order.
__global__ __launch_bounds__(SDR_THREADS) void sdr_fir_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, const int* __restrict__ lengths,
    int T, int n, int nfspans, const double* __restrict__ stage, double* __restrict__ fpart) {
  __shared__ double2 sD2[(SEGAN_SDR_SPAN + SEGAN_SDR_MAX_TAPS) / 2];
  __shared__ double2 cs2[SEGAN_SDR_MAX_TAPS / 2];
  __shared__ double sh[SDR_THREADS / 64][2];
  double* sD = reinterpret_cast<double*>(sD2);
  double* cs = reinterpret_cast<double*>(cs2);
  const int r = blockIdx.y, tid = threadIdx.x;
  const int L = segan_row_samples(lengths, r, T);
  const long long total = L > 0 ? (long long)L + n - 1 : 0;
  const long long start = (long long)blockIdx.x * SEGAN_SDR_SPAN;
  if (start >= total) return;   // the whole workgroup, before any barrier
  const float* s = ref + (size_t)r * T;
  const float* x = deg + (size_t)r * T;
  const int P = (n + 1) & ~1;
  for (int i = tid; i < SEGAN_SDR_SPAN + P; i += SDR_THREADS) {
    const long long g = start - P + i;
    sD[i] = (g >= 0 && g < L) ? (double)s[g] : 0.0;
  }
  const double* c = stage + (size_t)r * sdr_stage_stride(n) + 2 * (size_t)n;
  for (int k = tid; k < SEGAN_SDR_MAX_TAPS; k += SDR_THREADS) cs[k] = k < n ? c[k] : 0.0;
  __syncthreads();

  double st[SDR_T_PER_THREAD];
#pragma unroll
  for (int i = 0; i < SDR_T_PER_THREAD; ++i) st[i] = 0.0;
  const double* base = sD + 2 * tid + P;   // an even index: s[start + 2 tid]
  for (int k = 0; k < n; k += 2) {
    const double2 ck = *reinterpret_cast<const double2*>(cs + k);
#pragma unroll
    for (int i = 0; i < SDR_T_PER_THREAD / 2; ++i) {
      const double* q = base + 2 * SDR_THREADS * i - k;
      const double2 hi = *reinterpret_cast<const double2*>(q);   // s[t - k], s[t + 1 - k]
      const double lo = q[-1];                                   // s[t - k - 1]
      st[2 * i] = fma(ck.x, hi.x, st[2 * i]);
      st[2 * i + 1] = fma(ck.x, hi.y, st[2 * i + 1]);
      st[2 * i] = fma(ck.y, lo, st[2 * i]);
      st[2 * i + 1] = fma(ck.y, hi.x, st[2 * i + 1]);
    }
  }
  double acc[2] = {0.0, 0.0};
#pragma unroll
  for (int i = 0; i < SDR_T_PER_THREAD; ++i) {
    const long long g = start + 2 * tid + 2 * SDR_THREADS * (i >> 1) + (i & 1);
    if (g < total) {
      const double e = (g < L ? (double)x[g] : 0.0) - st[i];
      acc[0] = fma(st[i], st[i], acc[0]);
      acc[1] = fma(e, e, acc[1]);
    }
  }
  block_sum_fixed<2>(acc, sh);
  if (tid == 0) {
    double* p = fpart + ((size_t)r * nfspans + blockIdx.x) * 2;
    p[0] = acc[0];
    p[1] = acc[1];
  }
}

// one wave per row: the row's FIR spans added (lanes over spans in strides of 64, then the
// butterfly), St and Ee into the stage block, the value with its special cases into row_out
__global__ __launch_bounds__(64) void sdr_final_kernel(
    const int* __restrict__ lengths, int T, int n, int nfspans, const double* __restrict__ fpart,
    double* __restrict__ stage, double* __restrict__ row_out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int L = segan_row_samples(lengths, r, T);
  int mine = L > 0 ? sdr_spans((long long)L + n - 1) : 0;
  if (mine > nfspans) mine = nfspans;
  double St = 0.0, Ee = 0.0;
  for (int b = lane; b < mine; b += 64) {
    const double* p = fpart + ((size_t)r * nfspans + b) * 2;
    St += p[0];
    Ee += p[1];
  }
  St = segan_wave_sum(St);
  Ee = segan_wave_sum(Ee);
  if (lane != 0) return;
  double* sg = stage + (size_t)r * sdr_stage_stride(n);
  sg[3 * (size_t)n + 1] = St;
  sg[3 * (size_t)n + 2] = Ee;
  double v;
  if (L == 0 || sg[0] == 0.0) v = NAN;
  else if (Ee == 0.0) v = St == 0.0 ? (double)NAN : (double)INFINITY;
  else if (St == 0.0) v = -(double)INFINITY;
  else v = 10.0 * log10(St / Ee);
  row_out[r] = v;
}

int launch_solver(const double* r, const double* d, size_t in_stride, double* c, size_t c_stride,
                  int* order_i, double* order_d, size_t order_stride, int rows, int n,
                  hipStream_t st) {
  hipLaunchKernelGGL(toeplitz_solve_kernel, dim3(ceil_div(rows, SDR_ROWS_PER_WG)),
                     dim3(SDR_THREADS), 0, st, r, d, in_stride, c, c_stride, order_i, order_d,
                     order_stride, rows, n);
  return segan_check_launch("toeplitz_solve_kernel");
}

bool sdr_sizes_ok(int rows, int T, int taps) {
  return rows > 0 && rows <= 65535 && T > 0 && taps >= 1 && taps <= SEGAN_SDR_MAX_TAPS;
}

}  // namespace

extern "C" int segan_sdr_dims(int rows, int T, int taps, long long* out) {
  SEGAN_REQUIRE(out, "sdr: NULL pointer");
  SEGAN_REQUIRE(sdr_sizes_ok(rows, T, taps), "sdr: bad sizes rows=%d T=%d taps=%d", rows, T, taps);
  const long long nspans = sdr_spans(T), nfspans = sdr_spans((long long)T + taps - 1);
  out[0] = SEGAN_SDR_SPAN;
  out[1] = nspans;
  out[2] = (long long)rows * (nspans * 2 * taps + nfspans * 2 + (long long)sdr_stage_stride(taps));
  return SEGAN_OK;
}

extern "C" int segan_sdr(const float* ref, const float* deg, const int* lengths, int rows, int T,
                         int taps, double* row_out, double* stages_out, double* ws, void* stream) {
  SEGAN_REQUIRE(ref && deg && row_out && ws, "sdr: NULL pointer");
  SEGAN_REQUIRE(sdr_sizes_ok(rows, T, taps), "sdr: bad sizes rows=%d T=%d taps=%d", rows, T, taps);
  const int n = taps, nspans = sdr_spans(T), nfspans = sdr_spans((long long)T + n - 1);
  double* part = ws;                                         // [rows][nspans][2n]
  double* fpart = part + (size_t)rows * nspans * 2 * n;      // [rows][nfspans][2]
  double* stage = stages_out ? stages_out : fpart + (size_t)rows * nfspans * 2;   // [rows][3n+3]
  const size_t stride = sdr_stage_stride(n);
  hipStream_t st = (hipStream_t)stream;

  const size_t lds = 2 * (size_t)sdr_corr_ext(n) * sizeof(double);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sdr_corr_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    segan_set_error("sdr: %zu bytes of LDS refused for sdr_corr_kernel", lds);
    return SEGAN_ELAUNCH;
  }
  hipLaunchKernelGGL(sdr_corr_kernel, dim3(nspans, rows), dim3(SDR_THREADS), lds, st, ref, deg,
                     lengths, T, n, nspans, part);
  if (int e = segan_check_launch("sdr_corr_kernel")) return e;
  hipLaunchKernelGGL(sdr_corr_sum_kernel, dim3(ceil_div(2 * n, SDR_THREADS), rows),
                     dim3(SDR_THREADS), 0, st, lengths, T, n, nspans, (const double*)part, stage);
  if (int e = segan_check_launch("sdr_corr_sum_kernel")) return e;
  if (int e = launch_solver(stage, stage + n, stride, stage + 2 * (size_t)n, stride, nullptr,
                            stage + 3 * (size_t)n, stride, rows, n, st))
    return e;
  hipLaunchKernelGGL(sdr_fir_kernel, dim3(nfspans, rows), dim3(SDR_THREADS), 0, st, ref, deg,
                     lengths, T, n, nfspans, (const double*)stage, fpart);
  if (int e = segan_check_launch("sdr_fir_kernel")) return e;
  hipLaunchKernelGGL(sdr_final_kernel, dim3(rows), dim3(64), 0, st, lengths, T, n, nfspans,
                     (const double*)fpart, stage, row_out);
  return segan_check_launch("sdr_final_kernel");
}

extern "C" int segan_toeplitz_solve(const double* r, const double* d, int rows, int n,
                                    double* c_out, int* order_out, void* stream) {
  SEGAN_REQUIRE(r && d && c_out && order_out, "toeplitz_solve: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && n >= 1 && n <= SEGAN_SDR_MAX_TAPS,
                "toeplitz_solve: bad sizes rows=%d n=%d", rows, n);
  return launch_solver(r, d, (size_t)n, c_out, (size_t)n, order_out, nullptr, 0, rows, n,
                       (hipStream_t)stream);
}
