// The WPE dereverberation baseline (scripts/wpe_oracle.py,
// include/segan_dereverb.h): variance-normalised delayed linear prediction per frequency bin of a
// single-channel STFT.  fp64 on fp32 or fp64 rows, per-row lengths, no atomics, no scratch, every
// sum over the frames in ascending t in every lane, so a row's result depends neither on T, nor on
// the other rows, nor on what lies past its length, nor on the frame tile.
//
//   wpe_analysis_kernel   one workgroup per (2^b frames, row): the windowed frames as 2^b
//                         interleaved sequences through the LDS Stockham transform of
//                         segan_fft_lds.h into Y [rows][F][nf of T], bin-major
//   wpe_filter_kernel     one workgroup per (bin, row): the bin's series in LDS (rows of more than
//                         SEGAN_WPE_TILE frames: streamed in tiles with a halo of delay + taps - 1
//                         frames), and per iteration lambda, the taps (taps + 1) / 2 entries of R
//                         and the taps of P (one lane slot per entry, ascending t), the Cholesky
//                         factor and both substitutions in LDS; then X = Y - g^H y~
//   wpe_synthesis_kernel  one workgroup per (2^b - 3 hops, row): the Hermitian extension of 2^b
//                         frames of X through the inverse transform, window and overlap-add of the
//                         four frames over each hop, the earlier frame first; also nframes and the
//                         OR of the bins' flags into status
#include "segan_fft_lds.h"
#include "../../include/segan_dereverb.h"

// every product and every sum rounds on its own; the fused multiply-adds are asked for by name
#pragma clang fp contract(off)

#define WPE_THREADS 256
#define WPE_MAX_T (1 << 24)
#define WPE_PAD 3                                   // frames before the first sample's own
#define WPE_MAX_ENTRIES (SEGAN_WPE_MAX_TAPS * (SEGAN_WPE_MAX_TAPS + 1) / 2 + SEGAN_WPE_MAX_TAPS)
#define WPE_SLOTS ((WPE_MAX_ENTRIES + WPE_THREADS - 1) / WPE_THREADS)
#define WPE_FLOOR 1e-10
#define WPE_LOADING 1e-10

static_assert(WPE_THREADS == FFT_THREADS, "wpe: the transform's workgroup");
static_assert(SEGAN_WPE_MAX_TAPS <= 64, "wpe: the substitutions run in one wave's worth of lanes");

namespace {

struct WpeRate {
  int N, H, F, lgN;
};

__host__ __device__ inline bool wpe_rate(int srate, WpeRate* d) {
  if (srate != 16000 && srate != 8000) return false;
  d->lgN = srate == 16000 ? 9 : 8;
  d->N = 1 << d->lgN;
  d->H = d->N / 4;
  d->F = d->N / 2 + 1;
  return true;
}

__host__ __device__ inline int wpe_frames(int L, const WpeRate& d) {
  return (L + d.H - 1) / d.H + WPE_PAD;
}

// a row the filter leaves alone
__host__ __device__ inline bool wpe_short(int L, int nf, int taps, int delay) {
  return L == 0 || nf <= delay + taps;
}

struct WpeTable {
  int device, srate;
  double* win;   // [N]
};
SeganDeviceTables<WpeTable> g_wpe_tables;

const WpeTable* wpe_table(int srate) {
  return g_wpe_tables.get(
      "wpe", [srate](const WpeTable& e) { return e.srate == srate; },
      [srate](WpeTable* e) {
        WpeRate d;
        wpe_rate(srate, &d);
        std::vector<double> w(d.N);
        for (int n = 0; n < d.N; ++n)
          w[n] = sqrt(0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)d.N));
        e->srate = srate;
        return segan_upload(&e->win, w, "wpe");
      });
}

template <typename Tin>
__global__ __launch_bounds__(WPE_THREADS) void wpe_analysis_kernel(
    const Tin* __restrict__ x, const int* __restrict__ lengths, int T, WpeRate dr, int nfmax,
    const double* __restrict__ win, const double2* __restrict__ tw, double2* __restrict__ Y) {
  __shared__ double2 sm[FFT_LDS_N];
  const int r = blockIdx.y, tid = threadIdx.x;
  const int lgb = FFT_LDS_LOG2 - dr.lgN, nb = 1 << lgb;
  const int j0 = blockIdx.x << lgb;
  const int L = segan_row_samples(lengths, r, T);
  const int nf = wpe_frames(L, dr);
  double2* Yr = Y + (size_t)r * dr.F * (size_t)nfmax;
  if (j0 >= nf) {   // the whole workgroup, before any barrier: frames past the row's own are zero
    for (int idx = tid; idx < dr.F * nb; idx += WPE_THREADS) {
      const int t = idx & (nb - 1), kk = idx >> lgb;
      if (j0 + t < nfmax) Yr[(size_t)kk * nfmax + j0 + t] = make_double2(0.0, 0.0);
    }
    return;
  }
  const Tin* xr = x + (size_t)r * T;
  for (int idx = tid; idx < FFT_LDS_N; idx += WPE_THREADS) {
    const int i = idx & (dr.N - 1), t = idx >> dr.lgN;
    const long long s = (long long)(j0 + t - WPE_PAD) * dr.H + i;
    const double v = (s >= 0 && s < L) ? win[i] * (double)xr[s] : 0.0;
    sm[(i << lgb) | t] = make_double2(v, 0.0);
  }
  __syncthreads();
  fft_lds_passes(sm, tw, dr.lgN, lgb, false);
  for (int idx = tid; idx < dr.F * nb; idx += WPE_THREADS) {
    const int t = idx & (nb - 1), kk = idx >> lgb;
    if (j0 + t < nfmax) Yr[(size_t)kk * nfmax + j0 + t] = sm[(kk << lgb) | t];
  }
}

// the largest of v over the workgroup, in every thread; exact whatever the order
__device__ __forceinline__ double wpe_block_max(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  __syncthreads();
  return v;
}

// X_t = Y_t - sum_a conj(g_a) Y_{t-D-a}, a ascending; ys[i] holds Y[t0 - halo + i] and tl = t - t0
__device__ __forceinline__ double2 wpe_predict(const double2* ys, const double2* gv, int tl, int K,
                                               int halo) {
  double ax = 0.0, ay = 0.0;
  for (int a = 0; a < K; ++a) {
    const double2 g = gv[a], v = ys[tl + K - 1 - a];
    ax = fma(g.y, v.y, fma(g.x, v.x, ax));
    ay = fma(-g.y, v.x, fma(g.x, v.y, ay));
  }
  const double2 y = ys[tl + halo];
  return make_double2(y.x - ax, y.y - ay);
}

// ys[0 .. halo + tile) <- Y[t0 - halo ..), zero before the first frame and from nf on; ends behind
// a barrier
__device__ __forceinline__ void wpe_load_tile(double2* ys, const double2* __restrict__ Yk, int t0,
                                              int halo, int tile, int nf) {
  for (int i = threadIdx.x; i < halo + tile; i += WPE_THREADS) {
    const int t = t0 - halo + i;
    ys[i] = (t >= 0 && t < nf) ? Yk[t] : make_double2(0.0, 0.0);
  }
  __syncthreads();
}

// Dynamic LDS, in this order: ys double2[halo + tile], Rm double2[K K] (R, then its Cholesky
// factor in the lower triangle with the real pivots on the diagonal), zv double2[K], gv
// double2[K], inv double[tile], red double[4].
__host__ __device__ inline size_t wpe_filter_lds(int tile, int K, int D) {
  return 16 * (size_t)(D + K - 1 + tile + K * K + 2 * K) + 8 * (size_t)tile + 32;
}

__global__ __launch_bounds__(WPE_THREADS) void wpe_filter_kernel(
    const int* __restrict__ lengths, int T, WpeRate dr, int nfmax, int tile, int K, int D,
    int iterations, const double2* __restrict__ Y, double2* __restrict__ X,
    double2* __restrict__ g_out, int* __restrict__ flags, int fstride) {
  extern __shared__ __attribute__((aligned(16))) char wpe_smem[];
  const int k = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int halo = D + K - 1;
  double2* ys = reinterpret_cast<double2*>(wpe_smem);
  double2* Rm = ys + halo + tile;
  double2* zv = Rm + K * K;
  double2* gv = zv + K;
  double* inv = reinterpret_cast<double*>(gv + K);
  double* red = inv + tile;

  const int L = segan_row_samples(lengths, r, T);
  const int nf = wpe_frames(L, dr);
  const double2* Yk = Y + ((size_t)r * dr.F + k) * (size_t)nfmax;
  double2* Xk = X + ((size_t)r * dr.F + k) * (size_t)nfmax;
  double2* gk = g_out ? g_out + ((size_t)r * dr.F + k) * (size_t)K : nullptr;
  if (wpe_short(L, nf, K, D)) {   // the whole workgroup, before any barrier
    for (int t = tid; t < nfmax; t += WPE_THREADS) Xk[t] = Yk[t];
    if (gk && tid < K) gk[tid] = make_double2(0.0, 0.0);
    if (tid == 0) flags[(size_t)r * fstride + k] = 0;
    return;
  }

  // the entries of this lane: e < K (K + 1) / 2 is R[a][b], a >= b; then P[a]
  const int nR = K * (K + 1) / 2, nE = nR + K;
  int offA[WPE_SLOTS], offB[WPE_SLOTS], dst[WPE_SLOTS];
  bool act[WPE_SLOTS];
#pragma unroll
  for (int s = 0; s < WPE_SLOTS; ++s) {
    const int e = tid + WPE_THREADS * s;
    act[s] = e < nE;
    int a = 0, b = 0;
    if (e < nR) {
      while ((a + 1) * (a + 2) / 2 <= e) ++a;
      b = e - a * (a + 1) / 2;
      offB[s] = K - 1 - b;
      dst[s] = a * K + b;
    } else {
      a = act[s] ? e - nR : 0;
      offB[s] = halo;           // Y_t itself
      dst[s] = -1 - a;
    }
    offA[s] = K - 1 - a;
  }

  const int ntiles = (nf + tile - 1) / tile;
  const bool resident = ntiles == 1;
  if (tid < K) gv[tid] = make_double2(0.0, 0.0);
  if (resident) wpe_load_tile(ys, Yk, 0, halo, tile, nf);
  else __syncthreads();
  int fail = 0;

  for (int it = 0; it < iterations; ++it) {
    // m = max_t |X_t|^2 with the filter of the iteration before
    double mx = 0.0;
    for (int ti = 0; ti < ntiles; ++ti) {
      const int t0 = ti * tile, cnt = min(tile, nf - t0);
      if (!resident) {
        __syncthreads();
        wpe_load_tile(ys, Yk, t0, halo, tile, nf);
      }
      for (int tl = tid; tl < cnt; tl += WPE_THREADS) {
        const double2 v = wpe_predict(ys, gv, tl, K, halo);
        mx = fmax(mx, fma(v.x, v.x, v.y * v.y));
      }
    }
    const double m = wpe_block_max(mx, red);
    bool stop = !(m > 0.0);
    if (!stop) {
      const double floor_p = WPE_FLOOR * m;
      double2 acc[WPE_SLOTS];
#pragma unroll
      for (int s = 0; s < WPE_SLOTS; ++s) acc[s] = make_double2(0.0, 0.0);
      for (int ti = 0; ti < ntiles; ++ti) {
        const int t0 = ti * tile, cnt = min(tile, nf - t0);
        if (!resident) {
          __syncthreads();
          wpe_load_tile(ys, Yk, t0, halo, tile, nf);
        }
        for (int tl = tid; tl < cnt; tl += WPE_THREADS) {
          const double2 v = wpe_predict(ys, gv, tl, K, halo);
          inv[tl] = 1.0 / fmax(fma(v.x, v.x, v.y * v.y), floor_p);
        }
        __syncthreads();
        for (int tl = 0; tl < cnt; ++tl) {
          const double w = inv[tl];
#pragma unroll
          for (int s = 0; s < WPE_SLOTS; ++s) {
            if (act[s]) {
              const double2 ya = ys[tl + offA[s]], yb = ys[tl + offB[s]];
              const double pr = fma(ya.x, yb.x, ya.y * yb.y);
              const double pi = fma(ya.y, yb.x, -(ya.x * yb.y));
              acc[s].x = fma(pr, w, acc[s].x);
              acc[s].y = fma(pi, w, acc[s].y);
            }
          }
        }
      }
      __syncthreads();   // the last reads of gv by wpe_predict are behind: zv and Rm are free
#pragma unroll
      for (int s = 0; s < WPE_SLOTS; ++s) {
        if (act[s]) {
          if (dst[s] >= 0) {
            const bool diag = dst[s] % (K + 1) == 0;
            Rm[dst[s]] = make_double2(acc[s].x, diag ? 0.0 : acc[s].y);
          } else {
            zv[-1 - dst[s]] = acc[s];
          }
        }
      }
      __syncthreads();
      double tr = 0.0;
      for (int a = 0; a < K; ++a) tr += Rm[a * (K + 1)].x;
      stop = !(tr > 0.0);
      if (!stop) {
        const double load = WPE_LOADING * (tr / (double)K);
        __syncthreads();   // every thread has read the diagonal
        if (tid < K) Rm[tid * (K + 1)].x += load;
        __syncthreads();
        // R = L L^H, column by column: the pivot in every thread, row j + 1 + tid in its thread
        bool bad = false;
        for (int j = 0; j < K; ++j) {
          double d = Rm[j * (K + 1)].x;
          for (int c = 0; c < j; ++c) {
            const double2 l = Rm[j * K + c];
            d = d - fma(l.x, l.x, l.y * l.y);
          }
          bad = bad || !(d > 0.0);
          const double ljj = sqrt(d);
          const int i = j + 1 + tid;
          if (i < K) {
            double2 s = Rm[i * K + j];
            for (int c = 0; c < j; ++c) {
              const double2 li = Rm[i * K + c], lj = Rm[j * K + c];
              s.x = fma(-li.x, lj.x, fma(-li.y, lj.y, s.x));
              s.y = fma(-li.y, lj.x, fma(li.x, lj.y, s.y));
            }
            Rm[i * K + j] = make_double2(s.x / ljj, s.y / ljj);
          }
          __syncthreads();
          if (tid == 0) Rm[j * (K + 1)] = make_double2(ljj, 0.0);
        }
        __syncthreads();
        // L z = P: thread i carries its right-hand side, z_c goes through zv[c]
        double2 rh = tid < K ? zv[tid] : make_double2(0.0, 0.0);
        __syncthreads();
        for (int c = 0; c < K; ++c) {
          if (tid == c) {
            const double dg = Rm[c * (K + 1)].x;
            zv[c] = make_double2(rh.x / dg, rh.y / dg);
          }
          __syncthreads();
          if (tid > c && tid < K) {
            const double2 l = Rm[tid * K + c], z = zv[c];
            rh.x = fma(-l.x, z.x, fma(l.y, z.y, rh.x));
            rh.y = fma(-l.x, z.y, fma(-l.y, z.x, rh.y));
          }
        }
        // L^H g = z
        rh = tid < K ? zv[tid] : make_double2(0.0, 0.0);
        for (int c = K - 1; c >= 0; --c) {
          if (tid == c) {
            const double dg = Rm[c * (K + 1)].x;
            gv[c] = make_double2(rh.x / dg, rh.y / dg);
          }
          __syncthreads();
          if (tid < c) {
            const double2 l = Rm[c * K + tid], g = gv[c];
            rh.x = fma(-l.x, g.x, fma(-l.y, g.y, rh.x));
            rh.y = fma(-l.x, g.y, fma(l.y, g.x, rh.y));
          }
        }
        if (bad) {
          fail = SEGAN_WPE_ST_PIVOT;
          stop = true;
        }
      }
    }
    if (stop) {   // uniform over the workgroup: g = 0 and the bin is left alone from here on
      __syncthreads();
      if (tid < K) gv[tid] = make_double2(0.0, 0.0);
      __syncthreads();
      break;
    }
    __syncthreads();
  }

  for (int ti = 0; ti < ntiles; ++ti) {
    const int t0 = ti * tile, cnt = min(tile, nf - t0);
    if (!resident) {
      __syncthreads();
      wpe_load_tile(ys, Yk, t0, halo, tile, nf);
    }
    for (int tl = tid; tl < cnt; tl += WPE_THREADS) Xk[t0 + tl] = wpe_predict(ys, gv, tl, K, halo);
  }
  for (int t = nf + tid; t < nfmax; t += WPE_THREADS) Xk[t] = make_double2(0.0, 0.0);
  if (gk && tid < K) gk[tid] = gv[tid];
  if (tid == 0) flags[(size_t)r * fstride + k] = fail;
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(WPE_THREADS) void wpe_synthesis_kernel(
    const Tin* __restrict__ x, const int* __restrict__ lengths, int T, WpeRate dr, int nfmax, int K,
    int D, const double* __restrict__ win, const double2* __restrict__ tw,
    const double2* __restrict__ X, const int* __restrict__ flags, int fstride,
    Tout* __restrict__ y, int* __restrict__ nframes, int* __restrict__ status) {
  __shared__ double2 sm[FFT_LDS_N];
  const int r = blockIdx.y, tid = threadIdx.x;
  const int N = dr.N, H = dr.H, F = dr.F;
  const int lgb = FFT_LDS_LOG2 - dr.lgN, nb = 1 << lgb, hb = nb - WPE_PAD;
  const int h0 = blockIdx.x * hb;
  const int L = segan_row_samples(lengths, r, T);
  const int nf = wpe_frames(L, dr);
  const bool copy = wpe_short(L, nf, K, D);
  if (blockIdx.x == 0 && tid == 0) {
    int st = 0;
    for (int kk = 0; kk < F; ++kk) st |= flags[(size_t)r * fstride + kk];
    nframes[r] = nf;
    status[r] = st;
  }
  const long long n0 = (long long)h0 * H;
  if (copy || n0 >= L) {   // the whole workgroup, before any barrier
    for (int idx = tid; idx < hb * H; idx += WPE_THREADS) {
      const long long n = n0 + idx;
      if (n < T) y[(size_t)r * T + n] = n < L ? (Tout)x[(size_t)r * T + n] : (Tout)0;
    }
    return;
  }
  // frames h0 .. h0 + nb - 1, each with its Hermitian extension; t runs along memory
  const double2* Xr = X + (size_t)r * F * (size_t)nfmax;
  for (int idx = tid; idx < FFT_LDS_N; idx += WPE_THREADS) {
    const int t = idx & (nb - 1), kk = idx >> lgb;
    const int j = h0 + t;
    double2 v = make_double2(0.0, 0.0);
    if (j < nf) {
      if (kk < F) {
        v = Xr[(size_t)kk * nfmax + j];
        if (kk == 0 || kk == F - 1) v.y = 0.0;
      } else {
        v = Xr[(size_t)(N - kk) * nfmax + j];
        v.y = -v.y;
      }
    }
    sm[idx] = v;
  }
  __syncthreads();
  fft_lds_passes(sm, tw, dr.lgN, lgb, true);
  const double inv_n = 1.0 / (double)N;
  for (int idx = tid; idx < hb * H; idx += WPE_THREADS) {
    const int hh = idx / H, i = idx - hh * H;
    const long long n = n0 + idx;
    if (n >= T) continue;
    double o = 0.0;
    if (n < L) {   // the frames h0 + hh .. h0 + hh + 3 < nf hold the sample at 3 H + i, .., i
      double acc = 0.0;
#pragma unroll
      for (int q = 0; q <= WPE_PAD; ++q) {
        const int off = (WPE_PAD - q) * H + i;
        acc += (sm[(off << lgb) | (hh + q)].x * inv_n) * win[off];
      }
      o = 0.5 * acc;
    }
    y[(size_t)r * T + n] = (Tout)o;
  }
}

bool wpe_sizes_ok(int rows, int T) {
  return rows > 0 && rows <= 65535 && T > 0 && T <= WPE_MAX_T;
}

bool wpe_params_ok(int taps, int delay) {
  return taps >= 1 && taps <= SEGAN_WPE_MAX_TAPS && delay >= 1 && delay <= SEGAN_WPE_MAX_DELAY;
}

int wpe_flag_stride(int F) { return round_up(F, 4); }

template <typename Tin>
int wpe_run(const Tin* x, const int* lengths, int rows, int T, const WpeRate& dr, int srate,
            int taps, int delay, int iterations, void* y, int y_dtype, int* nframes, int* status,
            double* Y_out, double* X_out, double* g_out, void* ws, hipStream_t st) {
  const WpeTable* tb = wpe_table(srate);
  const FftTable* ft = fft_table();
  if (!tb || !ft) return SEGAN_ELAUNCH;
  const int nfmax = wpe_frames(T, dr), F = dr.F, fstride = wpe_flag_stride(F);
  const size_t spec = (size_t)rows * F * (size_t)nfmax;
  double2* Y = Y_out ? (double2*)Y_out : (double2*)ws;
  double2* X = X_out ? (double2*)X_out : (double2*)ws + spec;
  int* flags = (int*)((double2*)ws + 2 * spec);
  const int lgb = FFT_LDS_LOG2 - dr.lgN, nb = 1 << lgb;
  hipLaunchKernelGGL(wpe_analysis_kernel<Tin>, dim3(ceil_div(nfmax, nb), rows), dim3(WPE_THREADS),
                     0, st, x, lengths, T, dr, nfmax, (const double*)tb->win,
                     (const double2*)ft->tw, Y);
  if (int e = segan_check_launch("wpe_analysis_kernel")) return e;
  const int tile = nfmax < SEGAN_WPE_TILE ? nfmax : SEGAN_WPE_TILE;
  hipLaunchKernelGGL(wpe_filter_kernel, dim3(F, rows), dim3(WPE_THREADS),
                     wpe_filter_lds(tile, taps, delay), st, lengths, T, dr, nfmax, tile, taps,
                     delay, iterations, (const double2*)Y, X, (double2*)g_out, flags, fstride);
  if (int e = segan_check_launch("wpe_filter_kernel")) return e;
  const dim3 grid(ceil_div(ceil_div(T, dr.H), nb - WPE_PAD), rows), block(WPE_THREADS);
  if (y_dtype == SEGAN_DT_F64)
    hipLaunchKernelGGL((wpe_synthesis_kernel<Tin, double>), grid, block, 0, st, x, lengths, T, dr,
                       nfmax, taps, delay, (const double*)tb->win, (const double2*)ft->tw,
                       (const double2*)X, (const int*)flags, fstride, (double*)y, nframes, status);
  else
    hipLaunchKernelGGL((wpe_synthesis_kernel<Tin, float>), grid, block, 0, st, x, lengths, T, dr,
                       nfmax, taps, delay, (const double*)tb->win, (const double2*)ft->tw,
                       (const double2*)X, (const int*)flags, fstride, (float*)y, nframes, status);
  return segan_check_launch("wpe_synthesis_kernel");
}

}  // namespace

extern "C" int segan_wpe_dims(int rows, int T, int srate, int taps, int delay, long long* out) {
  WpeRate dr;
  SEGAN_REQUIRE(out, "wpe: NULL pointer");
  SEGAN_REQUIRE(wpe_sizes_ok(rows, T) && wpe_rate(srate, &dr),
                "wpe: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  SEGAN_REQUIRE(wpe_params_ok(taps, delay), "wpe: taps=%d is not in 1 .. %d or delay=%d not in 1 .. %d",
                taps, SEGAN_WPE_MAX_TAPS, delay, SEGAN_WPE_MAX_DELAY);
  const int nfmax = wpe_frames(T, dr);
  out[0] = dr.N;
  out[1] = dr.H;
  out[2] = dr.F;
  out[3] = nfmax;
  out[4] = (long long)rows * (32LL * dr.F * nfmax + 4LL * wpe_flag_stride(dr.F));
  return SEGAN_OK;
}

extern "C" int segan_wpe(const void* x, int x_dtype, const int* lengths, int rows, int T, int srate,
                         int taps, int delay, int iterations, void* y, int y_dtype, int* nframes,
                         int* status, double* Y_out, double* X_out, double* g_out, void* ws,
                         void* stream) {
  WpeRate dr;
  SEGAN_REQUIRE(x && y && nframes && status && ws, "wpe: NULL pointer");
  SEGAN_REQUIRE(wpe_sizes_ok(rows, T) && wpe_rate(srate, &dr),
                "wpe: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  SEGAN_REQUIRE(wpe_params_ok(taps, delay), "wpe: taps=%d is not in 1 .. %d or delay=%d not in 1 .. %d",
                taps, SEGAN_WPE_MAX_TAPS, delay, SEGAN_WPE_MAX_DELAY);
  SEGAN_REQUIRE(iterations >= 0 && iterations <= SEGAN_WPE_MAX_ITERATIONS,
                "wpe: iterations=%d is not in 0 .. %d", iterations, SEGAN_WPE_MAX_ITERATIONS);
  SEGAN_REQUIRE((x_dtype == SEGAN_DT_F32 || x_dtype == SEGAN_DT_F64) &&
                    (y_dtype == SEGAN_DT_F32 || y_dtype == SEGAN_DT_F64),
                "wpe: x and y are SEGAN_DT_F32 or SEGAN_DT_F64, got %d and %d", x_dtype, y_dtype);
  SEGAN_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)Y_out & 15) == 0 &&
                    ((uintptr_t)X_out & 15) == 0 && ((uintptr_t)g_out & 15) == 0,
                "wpe: the workspace and the stage outputs are not 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (x_dtype == SEGAN_DT_F64)
    return wpe_run((const double*)x, lengths, rows, T, dr, srate, taps, delay, iterations, y,
                   y_dtype, nframes, status, Y_out, X_out, g_out, ws, st);
  return wpe_run((const float*)x, lengths, rows, T, dr, srate, taps, delay, iterations, y, y_dtype,
                 nframes, status, Y_out, X_out, g_out, ws, st);
}
