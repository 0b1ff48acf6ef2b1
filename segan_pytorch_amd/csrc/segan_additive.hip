// segan_additive.hip — on-the-fly additive noise at a target SNR (the
// reference's `Additive`, segan/utils.py:43-297; the numpy oracle is scripts/additive_oracle.py):
//   * segan_asl_p56: the ITU-T P.56 method-B active speech level of rows of fp32 samples;
//   * segan_additive_mix: clean + sf * noise segment at the requested SNR, then the reference's
//     anti-clipping divisions.
// fp64 arithmetic on fp32 inputs, one workgroup per row, no atomics: every sum and scan runs in a
// fixed order that depends only on the row's own data, so a row's result does not depend on the
// other rows or on its position in the batch.  Products and sums that the reference rounds
// separately stay separate here (no contraction into fma unless written as fma).
#include "segan_signal.h"

#pragma clang fp contract(off)

#define AD_THREADS 256
#define AD_WAVES (AD_THREADS / 64)
#define AD_E 8             // consecutive samples per thread and slab
#define AD_NTHR 15         // thresholds 2^-15 .. 2^-1 (nbits = 16)
#define AD_INTERP_CAP 1000 // bin_interp iterations (the reference's loop has no bound)
#define AD_CLIP_CAP 1000   // anti-clipping divisions
#define AD_ST_CAP 1        // status bit: an iteration cap was reached
#define AD_ST_PN0 2        // status bit: the noise segment is digital silence (sf = 0)
#define AD_ST_RANGE 4      // status bit: segment outside the bank (sf = 0, nothing read)

namespace {

// sum over the workgroup in a fixed order (lanes by butterfly, then waves 0..3); every thread
// gets the result.  `sh` holds AD_WAVES doubles; reusable after the call returns.
__device__ __forceinline__ double ad_block_sum(double v, double* sh) {
  v = segan_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int w = 1; w < AD_WAVES; ++w) s += sh[w];
  return s;
}

// One-pole recurrence y[n] = g y[n-1] + u[n] across the workgroup.  Thread t ran its samples
// from a zero state and holds (a, b) = (g^count, final response); returns the state entering
// its first sample and advances `carry` (the row's state, replicated in every thread) past the
// slab.  Composition (a2, b2) o (a1, b1) = (a2 a1, a2 b1 + b2): shuffles inside a wave, then the
// four wave totals in order.
__device__ __forceinline__ double ad_scan_state(double a, double b, double& carry, double* wa,
                                                double* wb) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double pa = __shfl_up(a, o, 64), pb = __shfl_up(b, o, 64);
    if (lane >= o) {
      b = a * pb + b;
      a = a * pa;
    }
  }
  const double ea = __shfl_up(a, 1, 64), eb = __shfl_up(b, 1, 64);   // lane - 1's inclusive
  __syncthreads();   // wa / wb of the previous scan have been read
  if (lane == 63) {
    wa[wave] = a;
    wb[wave] = b;
  }
  __syncthreads();
  double s = carry, in = carry;
#pragma unroll
  for (int w = 0; w < AD_WAVES; ++w) {
    if (w == wave) in = s;
    s = wa[w] * s + wb[w];
  }
  carry = s;
  return lane == 0 ? in : ea * in + eb;
}

struct AslResult {
  double asl_ms, asl, c0;
  int status;
};

// utils.py:255-297, literally; the iteration cap is ours (the reference spins on NaN).
__device__ void ad_bin_interp(double upcount, double lwcount, double upthr, double lwthr,
                              double margin, double tol, double* out_log, double* out_thr,
                              int* status) {
  if (tol < 0) tol = -tol;
  int iterno = 1;
  if (fabs(upcount - upthr - margin) < tol || fabs(lwcount - lwthr - margin) < tol) {
    *out_log = lwcount;
    *out_thr = lwthr;
    return;
  }
  double midcount = (upcount + lwcount) / 2;
  double midthr = (upthr + lwthr) / 2;
  while (true) {
    const double diff = midcount - midthr - margin;
    if (fabs(diff) <= tol) break;
    iterno += 1;
    if (iterno > AD_INTERP_CAP) {
      *status |= AD_ST_CAP;
      break;
    }
    if (iterno > 20) tol *= 1.1;
    if (diff > tol) {
      midcount = (upcount + midcount) / 2;
      midthr = (upthr + midthr) / 2;
    } else if (diff < -tol) {
      midcount = (midcount - lwcount) / 2;   // as the reference writes it
      midthr = (midthr + lwthr) / 2;
    }
  }
  *out_log = midcount;
  *out_thr = midthr;
}

// utils.py:216-253 on the row's energy, activity counts and length
__device__ AslResult ad_finalise(double sq, const int* a, int len) {
  const double eps = 1e-22, M = 15.9;
  AslResult r;
  r.asl_ms = 0.0;
  r.asl = 0.0;
  r.c0 = NAN;
  r.status = 0;
  if (a[0] == 0) return r;
  double AdB[AD_NTHR], CdB[AD_NTHR];
  AdB[0] = 10 * log10(sq / (double)a[0] + eps);
  CdB[0] = 20 * log10(ldexp(1.0, -15) + eps);
  if (AdB[0] - CdB[0] < M) return r;
  for (int j = 1; j < AD_NTHR; ++j) {
    AdB[j] = 10 * log10(sq / ((double)a[j] + eps) + eps);
    CdB[j] = 20 * log10(ldexp(1.0, j - 15) + eps);
  }
  for (int j = 1; j < AD_NTHR; ++j) {
    if (a[j] != 0) {
      const double delta = AdB[j] - CdB[j];
      if (delta <= M) {
        double ms_log, cl0;
        ad_bin_interp(AdB[j], AdB[j - 1], CdB[j], CdB[j - 1], M, 0.5, &ms_log, &cl0, &r.status);
        r.asl_ms = pow(10.0, ms_log / 10);
        r.asl = (sq / (double)len) / r.asl_ms;
        r.c0 = pow(10.0, cl0 / 20);
        break;
      }
    }
  }
  return r;
}

}  // namespace

// ---------------------------------------------------------------------------------
// Active speech level.  A row is walked in slabs of 256 threads x AD_E samples:
//   p = one-pole(|x|), q = one-pole(p)  (y[n] = (1-g) u[n] + g y[n-1]) as two blocked scans;
//   per threshold c_j = 2^(j-15) the index of the last sample with q >= c_j (max-scan), and the
//   count a_j of samples at most `hang` samples after such an index: the reference's hangover
//   loop (utils.py:206-215) counts exactly the exceedance set dilated `hang` samples to the right.
// Thread 0 then finalises.  level[r] = (sq, asl_ms, asl, c0).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(AD_THREADS) void asl_p56_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, double* __restrict__ level,
    int* __restrict__ counts, int* __restrict__ status, double* __restrict__ qout, int T, double g,
    int hang) {
  __shared__ double wa[AD_WAVES], wb[AD_WAVES], wsum[AD_WAVES];
  __shared__ int wlast[AD_WAVES][AD_NTHR];
  __shared__ int wcnt[AD_WAVES][AD_NTHR];
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int L = segan_row_samples(lengths, r, T);
  const float* xr = x + (size_t)r * T;
  double* qr = qout ? qout + (size_t)r * T : nullptr;

  double gpow[AD_E + 1];
  gpow[0] = 1.0;
#pragma unroll
  for (int e = 1; e <= AD_E; ++e) gpow[e] = gpow[e - 1] * g;
  const double b0 = 1.0 - g;

  double sq = 0.0, carry_p = 0.0, carry_q = 0.0;
  int last_in[AD_NTHR], cnt[AD_NTHR];
#pragma unroll
  for (int j = 0; j < AD_NTHR; ++j) {
    last_in[j] = -1;   // the row's last exceeding index before this slab (none yet)
    cnt[j] = 0;
  }

  for (int base = 0; base < L; base += AD_THREADS * AD_E) {
    const int i0 = base + t * AD_E;
    const int n = L - i0 < 0 ? 0 : (L - i0 > AD_E ? AD_E : L - i0);
    double v[AD_E];
    double s = 0.0;
#pragma unroll
    for (int e = 0; e < AD_E; ++e) {
      if (e < n) {
        const double xv = (double)xr[i0 + e];
        sq = fma(xv, xv, sq);
        s = b0 * fabs(xv) + g * s;
      }
      v[e] = s;
    }
    double cin = ad_scan_state(gpow[n], s, carry_p, wa, wb);
    s = 0.0;
#pragma unroll
    for (int e = 0; e < AD_E; ++e) {
      if (e < n) {
        const double p = v[e] + gpow[e + 1] * cin;
        s = b0 * p + g * s;
      }
      v[e] = s;
    }
    cin = ad_scan_state(gpow[n], s, carry_q, wa, wb);

    // q of this thread's samples, and its own last exceeding index per threshold
    int last[AD_NTHR];
#pragma unroll
    for (int j = 0; j < AD_NTHR; ++j) last[j] = -1;
#pragma unroll
    for (int e = 0; e < AD_E; ++e) {
      if (e < n) {
        v[e] = v[e] + gpow[e + 1] * cin;
        if (qr) qr[i0 + e] = v[e];
#pragma unroll
        for (int j = 0; j < AD_NTHR; ++j)
          if (v[e] >= ldexp(1.0, j - 15)) last[j] = i0 + e;
      }
    }
    // exclusive max-scan of `last` over the threads before this one, on top of last_in
    int excl[AD_NTHR];
#pragma unroll
    for (int j = 0; j < AD_NTHR; ++j) {
      int m = last[j];
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int pm = __shfl_up(m, o, 64);
        if (lane >= o) m = pm > m ? pm : m;
      }
      const int em = __shfl_up(m, 1, 64);
      excl[j] = lane == 0 ? -1 : em;
      if (lane == 63) wlast[wave][j] = m;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < AD_NTHR; ++j) {
      int in = last_in[j], tot = last_in[j];
#pragma unroll
      for (int w = 0; w < AD_WAVES; ++w) {
        const int wl = wlast[w][j];
        if (w < wave) in = wl > in ? wl : in;
        tot = wl > tot ? wl : tot;
      }
      last_in[j] = tot;
      int cur = excl[j] > in ? excl[j] : in;
      int c = 0;
#pragma unroll
      for (int e = 0; e < AD_E; ++e) {
        if (e < n) {
          if (v[e] >= ldexp(1.0, j - 15)) cur = i0 + e;
          c += (cur >= 0 && i0 + e - cur <= hang) ? 1 : 0;
        }
      }
      cnt[j] += c;
    }
    __syncthreads();   // wlast has been read
  }
  if (qr)
    for (int i = L + t; i < T; i += AD_THREADS) qr[i] = 0.0;

  sq = ad_block_sum(sq, wsum);
#pragma unroll
  for (int j = 0; j < AD_NTHR; ++j) {
    int c = cnt[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) wcnt[wave][j] = c;
  }
  __syncthreads();
  if (t == 0) {
    int a[AD_NTHR];
    for (int j = 0; j < AD_NTHR; ++j) {
      a[j] = 0;
      for (int w = 0; w < AD_WAVES; ++w) a[j] += wcnt[w][j];
      counts[(size_t)r * AD_NTHR + j] = a[j];
    }
    const AslResult res = ad_finalise(sq, a, L);
    double* lv = level + (size_t)r * 4;
    lv[0] = sq;
    lv[1] = res.asl_ms;
    lv[2] = res.asl;
    lv[3] = res.c0;
    status[r] = res.status;
  }
}

// ---------------------------------------------------------------------------------
// Mix.  Per row: Pn = mean square of the segment bank[start .. start + L), sf = sqrt(Px / Pn /
// 10^(snr/10)), v = clean + sf * segment in fp64; the anti-clipping loop of utils.py:89-95 runs on
// the row's (max, min) — division by a positive number is monotone — to find the number of
// divisions n, and every sample takes the same n successive divisions by 1.1, 1.2, ... (small
// += 0.1 in fp64, never a product of divisors) before it is rounded to fp32 once.  `prev` (the
// clean sample preceding the row, for a pre-emphasis that follows) is mixed with bank[start - 1]
// the same way.  info[r] = (Pn, sf), istat[r] = (n, status).
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(AD_THREADS) void additive_mix_kernel(
    const float* __restrict__ clean, const int* __restrict__ lengths,
    const float* __restrict__ bank, long long n_bank, const long long* __restrict__ starts,
    const double* __restrict__ snr_db, const double* __restrict__ px,
    const float* __restrict__ prev, float* __restrict__ noisy, float* __restrict__ prev_out,
    double* __restrict__ info, int* __restrict__ istat, int T) {
  __shared__ double wsum[AD_WAVES], wmax[AD_WAVES], wmin[AD_WAVES];
  __shared__ int wnan[AD_WAVES];
  const int r = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int L = segan_row_samples(lengths, r, T);
  const float* cr = clean + (size_t)r * T;
  float* out = noisy + (size_t)r * T;
  const long long s0 = starts[r];
  const long long lo = prev ? s0 - 1 : s0;
  int st = 0;
  if (lo < 0 || s0 > n_bank || (long long)L > n_bank - s0) st |= AD_ST_RANGE;
  const float* seg = bank + (st ? 0 : s0);   // never dereferenced when out of range

  double acc = 0.0;
  if (!st)
    for (int i = t; i < L; i += AD_THREADS) {
      const double z = (double)seg[i];
      acc = fma(z, z, acc);
    }
  acc = ad_block_sum(acc, wsum);
  const double Pn = L > 0 ? acc / (double)L : 0.0;
  if (!st && !(Pn > 0.0) && !(Pn != Pn)) st |= AD_ST_PN0;
  double sf = 0.0;
  if (!st) sf = sqrt(px[r] / Pn / pow(10.0, snr_db[r] / 10));

  double mx = -INFINITY, mn = INFINITY;
  int has_nan = 0;
  for (int i = t; i < L; i += AD_THREADS) {
    const double z = st ? 0.0 : (double)seg[i];
    const double v = (double)cr[i] + z * sf;
    has_nan |= v != v;
    mx = fmax(mx, v);
    mn = fmin(mn, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mx = fmax(mx, __shfl_xor(mx, o, 64));
    mn = fmin(mn, __shfl_xor(mn, o, 64));
    has_nan |= __shfl_xor(has_nan, o, 64);
  }
  if (lane == 0) {
    wmax[wave] = mx;
    wmin[wave] = mn;
    wnan[wave] = has_nan;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < AD_WAVES; ++w) {
    mx = fmax(mx, wmax[w]);
    mn = fmin(mn, wmin[w]);
    has_nan |= wnan[w];
  }
  // numpy's max / min of a row with a NaN are NaN: both comparisons false, no division
  int n = 0;
  if (!has_nan && L > 0) {
    double small = 0.1;
    while (mx >= 1.0 || mn < -1.0) {
      if (n >= AD_CLIP_CAP) {
        st |= AD_ST_CAP;
        break;
      }
      const double d = 1.0 + small;
      mx = mx / d;
      mn = mn / d;
      small = small + 0.1;
      ++n;
    }
  }
  for (int i = t; i < T + (prev ? 1 : 0); i += AD_THREADS) {
    if (i >= L && i < T) {
      out[i] = cr[i];   // past the row's own length: unchanged
      continue;
    }
    const bool is_prev = i == T;
    const double z = st ? 0.0 : (double)(is_prev ? seg[-1] : seg[i]);
    double v = (double)(is_prev ? prev[r] : cr[i]) + z * sf;
    double small = 0.1;
    for (int k = 0; k < n; ++k) {
      v = v / (1.0 + small);
      small = small + 0.1;
    }
    if (is_prev)
      prev_out[r] = (float)v;
    else
      out[i] = (float)v;
  }
  if (t == 0) {
    info[2 * (size_t)r] = Pn;
    info[2 * (size_t)r + 1] = sf;
    istat[2 * (size_t)r] = n;
    istat[2 * (size_t)r + 1] = st;
  }
}

// ---------------------------------------------------------------------------------
// The loader's side of the mixer (datasets.PCMShardLoader): the clean row of selected shard items
// as the fp32 min-max-normalised wave (se_dataset.py:108-117; element 0 of a stored row is the
// sample preceding the slice -> prev), and the pre-emphasis of the mixed rows written over the
// selected items' noisy rows, in double and rounded once like segan_pcm16_prep.  index[k] is the
// batch item of row k (NULL: k); items outside 0 .. B-1 are skipped.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(AD_THREADS) void pcm16_wave_kernel(
    const int16_t* __restrict__ pcm, const int* __restrict__ index, float* __restrict__ wave,
    float* __restrict__ prev, int B, int T) {
  const int k = blockIdx.y;
  const int b = index ? index[k] : k;
  if (b < 0 || b >= B) return;
  const int16_t* src = pcm + (size_t)b * 2 * (T + 1);
  for (int i = blockIdx.x * AD_THREADS + threadIdx.x; i <= T; i += gridDim.x * AD_THREADS) {
    const float v = (float)((2.0 / 65535.0) * ((double)src[i] - 32767.0) + 1.0);
    if (i == 0)
      prev[k] = v;
    else
      wave[(size_t)k * T + i - 1] = v;
  }
}

__global__ __launch_bounds__(AD_THREADS) void preemph_rows_kernel(
    const float* __restrict__ x, const float* __restrict__ prev,
    const unsigned char* __restrict__ first, const int* __restrict__ index, float* __restrict__ y,
    int B, int T, double coef) {
  const int k = blockIdx.y;
  const int b = index ? index[k] : k;
  if (b < 0 || b >= B) return;
  const float* xr = x + (size_t)k * T;
  float* yr = y + (size_t)b * T;
  const bool starts_wav = first[b] != 0;
  for (int i = blockIdx.x * AD_THREADS + threadIdx.x; i < T; i += gridDim.x * AD_THREADS) {
    double v = (double)xr[i];
    if (coef > 0.0 && !(i == 0 && starts_wav))
      v = v - coef * (double)(i == 0 ? prev[k] : xr[i - 1]);
    yr[i] = (float)v;
  }
}

extern "C" int segan_asl_p56(const float* x, const int* lengths, int rows, int T, int srate,
                             int nbits, double* level, int* counts, int* status, double* q,
                             void* stream) {
  SEGAN_REQUIRE(x && level && counts && status, "asl_p56: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && T > 0 && (long long)T <= (1ll << 30), "asl_p56: bad sizes rows=%d T=%d",
                rows, T);
  SEGAN_REQUIRE(srate > 0 && srate <= 768000, "asl_p56: bad srate %d", srate);
  if (nbits != AD_NTHR + 1) {
    segan_set_error("asl_p56: nbits=%d is not supported (16 only)", nbits);
    return SEGAN_EUNSUPPORTED;
  }
  const double g = exp(-1.0 / ((double)srate * 0.03));
  const int hang = (int)ceil((double)srate * 0.2);
  hipLaunchKernelGGL(asl_p56_kernel, dim3(rows), dim3(AD_THREADS), 0, (hipStream_t)stream, x,
                     lengths, level, counts, status, q, T, g, hang);
  return segan_check_launch("asl_p56_kernel");
}

extern "C" int segan_additive_mix(const float* clean, const int* lengths, const float* bank,
                                  int64_t n_bank, const int64_t* starts, const double* snr_db,
                                  const double* px, const float* prev, int rows, int T,
                                  float* noisy, float* prev_out, double* info, int* istat,
                                  void* stream) {
  SEGAN_REQUIRE(clean && bank && starts && snr_db && px && noisy && info && istat,
                "additive_mix: NULL pointer");
  SEGAN_REQUIRE((prev == nullptr) == (prev_out == nullptr),
                "additive_mix: prev and prev_out go together");
  SEGAN_REQUIRE(rows > 0 && T > 0 && n_bank > 0, "additive_mix: bad sizes rows=%d T=%d bank=%lld",
                rows, T, (long long)n_bank);
  hipLaunchKernelGGL(additive_mix_kernel, dim3(rows), dim3(AD_THREADS), 0, (hipStream_t)stream,
                     clean, lengths, bank, (long long)n_bank, (const long long*)starts, snr_db, px,
                     prev, noisy, prev_out, info, istat, T);
  return segan_check_launch("additive_mix_kernel");
}

extern "C" int segan_pcm16_wave(const int16_t* pcm, const int* index, float* wave, float* prev,
                                int n, int B, int T, void* stream) {
  SEGAN_REQUIRE(pcm && wave && prev, "pcm16_wave: NULL pointer");
  SEGAN_REQUIRE(n > 0 && n <= 65535 && B > 0 && T > 0, "pcm16_wave: bad sizes n=%d B=%d T=%d", n,
                B, T);
  const int bx = ceil_div(T + 1, AD_THREADS) > 64 ? 64 : ceil_div(T + 1, AD_THREADS);
  hipLaunchKernelGGL(pcm16_wave_kernel, dim3(bx, n), dim3(AD_THREADS), 0, (hipStream_t)stream, pcm,
                     index, wave, prev, B, T);
  return segan_check_launch("pcm16_wave_kernel");
}

extern "C" int segan_preemph_rows(const float* x, const float* prev, const unsigned char* first,
                                  const int* index, float* y, int n, int B, int T, double coef,
                                  void* stream) {
  SEGAN_REQUIRE(x && prev && first && y, "preemph_rows: NULL pointer");
  SEGAN_REQUIRE(n > 0 && n <= 65535 && B > 0 && T > 0, "preemph_rows: bad sizes n=%d B=%d T=%d", n,
                B, T);
  const int bx = ceil_div(T, AD_THREADS) > 64 ? 64 : ceil_div(T, AD_THREADS);
  hipLaunchKernelGGL(preemph_rows_kernel, dim3(bx, n), dim3(AD_THREADS), 0, (hipStream_t)stream, x,
                     prev, first, index, y, B, T, coef > 0.0 ? coef : 0.0);
  return segan_check_launch("preemph_rows_kernel");
}
