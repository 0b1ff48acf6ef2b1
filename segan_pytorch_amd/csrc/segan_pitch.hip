// Pitch tracking by YIN (de Cheveigne & Kawahara 2002) with a 5 ms hop, and the F0 / voicing
// measures taken on two such contours (scripts/pitch_oracle.py).  fp64 on
// fp32 rows, per-row lengths, no atomics, every sum in an order fixed by the indices alone, so a
// row's result depends neither on T, nor on the other rows, nor on what lies past its length, and
// a row times a power of two gives the same lags and the same f0 bits.
//
//   pitch_block_kernel  one workgroup per (PITCH_GROUP hop blocks, row), one thread per lag: the
//                       block sums S_u(tau) = sum x[j] x[j+tau], E_u(tau) = sum x[j+tau]^2 over the
//                       block's H samples j in ascending order (exact products of fp32 values)
//   pitch_frame_kernel  one workgroup per (PITCH_FRAMES frames, row): the five blocks of a frame
//                       added in ascending order, d, its ascending running sum c, d' = d tau / c,
//                       the pick, the parabola
//   f0_eval_kernel      one wave per row: the interpolated log-f0 contours of ref and deg and the
//                       row's sums in ascending frame order
#include "segan_signal.h"

// nothing below may be contracted: the oracle rounds every product and every sum on its own (the
// block sums ask for their fused multiply-adds by name; their products are exact)
#pragma clang fp contract(off)

#define PITCH_GROUP 8          // hop blocks per workgroup of pitch_block_kernel
#define PITCH_FRAMES 16        // frames per workgroup of pitch_frame_kernel
#define PITCH_THREADS 256
#define PITCH_LAG_PITCH 269    // odd: the frames' serial walks fall on different LDS banks

namespace {

// ws[row][nbmax][2][nl]: S then E of each hop block
__global__ __launch_bounds__(320) void pitch_block_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, int T, int H, int nl, int nbmax,
    double* __restrict__ ws) {
  __shared__ double xs[PITCH_GROUP * PITCH_MAX_H + PITCH_MAX_LAGS];
  const int r = blockIdx.y, tau = threadIdx.x;
  const int L = segan_row_samples(lengths, r, T);
  int nb = pitch_blocks(L, H, nl);
  if (nb > nbmax) nb = nbmax;
  const int u0 = blockIdx.x * PITCH_GROUP;
  if (u0 >= nb) return;   // the whole workgroup, before any barrier
  const int ng = nb - u0 < PITCH_GROUP ? nb - u0 : PITCH_GROUP;
  const int count = ng * H + nl - 1;   // at most PITCH_GROUP * PITCH_MAX_H + PITCH_MAX_LAGS - 1
  const float* xr = x + (size_t)r * T;
  const long long start = (long long)u0 * H;
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const long long g = start + i;
    xs[i] = g < L ? (double)xr[g] : 0.0;   // g < L by construction; the bound costs nothing
  }
  __syncthreads();
  if (tau >= nl) return;   // no barrier below
  for (int u = 0; u < ng; ++u) {
    const double* a = xs + u * H;
    const double* b = a + tau;
    double S = 0.0, E = 0.0;
    for (int j = 0; j < H; ++j) {
      const double bj = b[j];
      S = fma(a[j], bj, S);
      E = fma(bj, bj, E);
    }
    double* o = ws + ((size_t)r * nbmax + (u0 + u)) * 2 * (size_t)nl;
    o[tau] = S;
    o[nl + tau] = E;
  }
}

// Frames [16 blockIdx.x, + 16) of row blockIdx.y.  f0 / lag / ap [rows][F] and cmnd [rows][F][nl]
// may each be NULL; frames from the row's own count on get the fill values (cmnd: NaN).  ctot
// [rows][F] (NULL or c(tau_max + 1) of the row's own frames; the others are left alone).
__global__ __launch_bounds__(PITCH_THREADS) void pitch_frame_kernel(
    const int* __restrict__ lengths, int T, int srate, PitchRate pr, int nbmax, int F, double theta,
    const double* __restrict__ ws, double* __restrict__ f0, int* __restrict__ lag,
    double* __restrict__ ap, double* __restrict__ cmnd, double* __restrict__ ctot) {
  __shared__ double dd[PITCH_FRAMES][PITCH_LAG_PITCH];
  __shared__ double clast[PITCH_FRAMES];
  const int r = blockIdx.y, tid = threadIdx.x, nl = pr.nl;
  const int L = segan_row_samples(lengths, r, T);
  int nb = pitch_blocks(L, pr.H, nl);
  if (nb > nbmax) nb = nbmax;
  int nf = pitch_frames_of(nb);
  if (nf > F) nf = F;
  const int t0 = blockIdx.x * PITCH_FRAMES;
  const int tend = t0 + PITCH_FRAMES < F ? t0 + PITCH_FRAMES : F;
  const int nfr = nf - t0 < 0 ? 0 : (nf - t0 < PITCH_FRAMES ? nf - t0 : PITCH_FRAMES);

  // the frames past the row's own count
  const int first_fill = t0 + nfr;
  if (f0)
    for (int t = first_fill + tid; t < tend; t += PITCH_THREADS) {
      f0[(size_t)r * F + t] = 0.0;
      lag[(size_t)r * F + t] = -1;
      ap[(size_t)r * F + t] = NAN;
    }
  if (cmnd) {
    const long long n = (long long)(tend - first_fill) * nl;
    double* o = cmnd + ((size_t)r * F + first_fill) * (size_t)nl;
    for (long long i = tid; i < n; i += PITCH_THREADS) o[i] = NAN;
  }
  if (nfr == 0) return;   // the whole workgroup, before any barrier

  // d_t(tau) = (E_t(0) + E_t(tau)) - 2 R_t(tau), the blocks t .. t + 4 added in ascending order
  for (int i = tid; i < nfr * nl; i += PITCH_THREADS) {
    const int f = i / nl, tau = i - f * nl;
    const double* b = ws + ((size_t)r * nbmax + (t0 + f)) * 2 * (size_t)nl;
    double R = b[tau], E = b[nl + tau], E0 = b[nl];
#pragma unroll
    for (int u = 1; u < SEGAN_PITCH_NB; ++u) {
      const double* bu = b + (size_t)u * 2 * nl;
      R += bu[tau];
      E += bu[nl + tau];
      E0 += bu[nl];
    }
    dd[f][tau] = tau == 0 ? 0.0 : (E0 + E) - 2.0 * R;
  }
  __syncthreads();
  // c_t(tau), the ascending running sum, and d' = d tau / c: one thread per frame
  if (tid < nfr) {
    double c = 0.0;
    dd[tid][0] = 1.0;
    for (int tau = 1; tau < nl; ++tau) {
      const double v = dd[tid][tau];
      c += v;
      dd[tid][tau] = c > 0.0 ? v * (double)tau / c : 1.0;
    }
    clast[tid] = c;
    if (ctot) ctot[(size_t)r * F + t0 + tid] = c;
  }
  __syncthreads();
  if (cmnd)
    for (int i = tid; i < nfr * nl; i += PITCH_THREADS) {
      const int f = i / nl, tau = i - f * nl;
      cmnd[((size_t)r * F + t0 + f) * (size_t)nl + tau] = dd[f][tau];
    }
  if (tid >= nfr || !f0) return;
  const double* d = dd[tid];
  int tau = 0;
  if (clast[tid] > 0.0) {
    for (int k = pr.tmin; k <= pr.tmax; ++k)
      if (d[k] < theta) {
        tau = k;
        break;
      }
    if (tau)
      while (tau < pr.tmax && d[tau + 1] < d[tau]) ++tau;
  }
  double f = 0.0, a;
  if (tau) {
    const double ya = d[tau - 1], yb = d[tau], yc = d[tau + 1];
    const double den = ya - 2.0 * yb + yc;
    double delta = 0.0;
    if (den > 0.0) {
      delta = 0.5 * (ya - yc) / den;
      delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
    }
    f = (double)srate / ((double)tau + delta);
    a = yb;
  } else {
    a = d[pr.tmin];
    for (int k = pr.tmin + 1; k <= pr.tmax; ++k) a = d[k] < a ? d[k] : a;
  }
  const size_t o = (size_t)r * F + t0 + tid;
  f0[o] = f;
  lag[o] = tau;
  ap[o] = a;
}

// acc + v of lane 0 + v of lane 1 + ... + v of lane 63, the same bits in every lane
__device__ __forceinline__ double lanes_ascending(double acc, double v) {
  for (int i = 0; i < 64; ++i) acc += __shfl(v, i, 64);
  return acc;
}

// the first voiced frame at or after `from` (a multiple of 64), or -1: wave-uniform
__device__ __forceinline__ int next_voiced_chunk(const int* __restrict__ lag, int from, int nf,
                                                 int lane) {
  for (int b = from; b < nf; b += 64) {
    const int t = b + lane;
    const unsigned long long m = __ballot(t < nf && lag[t] > 0);
    if (m) return b + __ffsll((long long)m) - 1;
  }
  return -1;
}

// One contour's walk over the row's chunks of 64 frames: `last` is the last voiced frame before
// the chunk, `ahead` the first one after it (each -1 for none).
struct Contour {
  const double* f0;
  const int* lag;
  int last, ahead;
};

// log f0 of frame b + lane: its own where voiced, else on the line between the neighbouring voiced
// frames p < t < n, lp + (t - p) ((ln - lp) / (n - p)), else the nearest voiced frame's.  The row
// has a voiced frame.  Returns whether the frame is voiced through *uv; frames from nf on: 0.
__device__ __forceinline__ double contour_chunk(Contour& c, int b, int nf, int lane, bool* uv) {
  const int t = b + lane;
  const bool v = t < nf && c.lag[t] > 0;
  const unsigned long long m = __ballot(v);
  if (c.ahead < b + 64) c.ahead = next_voiced_chunk(c.lag, b + 64, nf, lane);
  const unsigned long long below = m & ((2ull << lane) - 1ull);          // lanes <= lane
  const unsigned long long above = m & ~((1ull << lane) - 1ull);         // lanes >= lane
  const int p = below ? b + 63 - __clzll((long long)below) : c.last;
  const int n = above ? b + __ffsll((long long)above) - 1 : c.ahead;
  double l = 0.0;
  if (t < nf) {
    if (p == t) {
      l = log(c.f0[t]);
    } else if (p < 0) {
      l = log(c.f0[n]);
    } else if (n < 0) {
      l = log(c.f0[p]);
    } else {
      const double lp = log(c.f0[p]), ln = log(c.f0[n]);
      l = lp + (double)(t - p) * ((ln - lp) / (double)(n - p));
    }
  }
  if (m) c.last = b + 63 - __clzll((long long)m);
  *uv = v;
  return l;
}

// out[row][4] = (f0_mae, vuv_acc, f0_kld, voiced)
__global__ __launch_bounds__(64) void f0_eval_kernel(
    const double* __restrict__ f0_ref, const int* __restrict__ lag_ref,
    const double* __restrict__ f0_deg, const int* __restrict__ lag_deg,
    const int* __restrict__ nframes, int F, double* __restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  int nf = nframes ? nframes[r] : F;
  nf = nf < 0 ? 0 : (nf > F ? F : nf);
  const double* fr = f0_ref + (size_t)r * F;
  const double* fd = f0_deg + (size_t)r * F;
  const int* lr = lag_ref + (size_t)r * F;
  const int* ld = lag_deg + (size_t)r * F;
  double* o = out + (size_t)r * 4;

  int vr = 0, vd = 0, same = 0;
  for (int b = 0; b < nf; b += 64) {
    const int t = b + lane;
    const bool in = t < nf, a = in && lr[t] > 0, d = in && ld[t] > 0;
    vr += __popcll(__ballot(a));
    vd += __popcll(__ballot(d));
    same += __popcll(__ballot(in && a == d));
  }
  const double nan = NAN;
  if (nf == 0) {
    if (lane < 4) o[lane] = nan;
    return;
  }
  const double acc = (double)same / (double)nf, voiced = (double)vr / (double)nf;
  if (vr == 0 || vd == 0) {
    if (lane == 0) {
      o[0] = nan;
      o[1] = acc;
      o[2] = nan;
      o[3] = voiced;
    }
    return;
  }
  double mae = 0.0, sr = 0.0, sd = 0.0;
  {
    Contour cr = {fr, lr, -1, -1};
    Contour cd = {fd, ld, -1, -1};
    for (int b = 0; b < nf; b += 64) {
      bool ur, ud;
      const double a = contour_chunk(cr, b, nf, lane, &ur);
      const double d = contour_chunk(cd, b, nf, lane, &ud);
      mae = lanes_ascending(mae, ur ? fabs(exp(d) - exp(a)) : 0.0);
      sr = lanes_ascending(sr, a);
      sd = lanes_ascending(sd, d);
    }
  }
  const double mr = sr / (double)nf, md = sd / (double)nf;
  double qr = 0.0, qd = 0.0;
  {
    Contour cr = {fr, lr, -1, -1};
    Contour cd = {fd, ld, -1, -1};
    for (int b = 0; b < nf; b += 64) {
      bool ur, ud;
      const double a = contour_chunk(cr, b, nf, lane, &ur);
      const double d = contour_chunk(cd, b, nf, lane, &ud);
      const bool in = b + lane < nf;
      qr = lanes_ascending(qr, in ? (a - mr) * (a - mr) : 0.0);
      qd = lanes_ascending(qd, in ? (d - md) * (d - md) : 0.0);
    }
  }
  if (lane != 0) return;
  double kld = nan;
  if (nf >= 2) {
    const double sg = sqrt(qr / (double)(nf - 1)), sp = sqrt(qd / (double)(nf - 1));
    if (sp != 0.0) {
      const double dm = md - mr;
      kld = log(sg / sp + 1e-22) + (sp * sp + dm * dm) / (2.0 * (sg * sg) + 1e-22) - 0.5;
    }
  }
  o[0] = mae / (double)vr;
  o[1] = acc;
  o[2] = kld;
  o[3] = voiced;
}

bool pitch_sizes_ok(int rows, int T) { return segan_pitch_sizes_ok(rows, T); }

// the two tracking stages; f0 / lag / ap or cmnd may be NULL
int pitch_run(const float* x, const int* lengths, int rows, int T, int srate, double theta,
              double* f0, int* lag, double* ap, double* cmnd, double* ctot, double* ws,
              hipStream_t st) {
  PitchRate pr;
  pitch_rate(srate, &pr);
  const int nbmax = pitch_blocks(T, pr.H, pr.nl), F = pitch_frames_of(nbmax);
  if (F == 0) return SEGAN_OK;   // no row has a frame: there is nothing to write
  hipLaunchKernelGGL(pitch_block_kernel, dim3(ceil_div(nbmax, PITCH_GROUP), rows),
                     dim3(round_up(pr.nl, 64)), 0, st, x, lengths, T, pr.H, pr.nl, nbmax, ws);
  if (int e = segan_check_launch("pitch_block_kernel")) return e;
  hipLaunchKernelGGL(pitch_frame_kernel, dim3(ceil_div(F, PITCH_FRAMES), rows),
                     dim3(PITCH_THREADS), 0, st, lengths, T, srate, pr, nbmax, F, theta,
                     (const double*)ws, f0, lag, ap, cmnd, ctot);
  return segan_check_launch("pitch_frame_kernel");
}

}  // namespace

int segan_pitch_cmnd_ctot(const float* x, const int* lengths, int rows, int T, int srate,
                          double* cmnd, double* ctot, double* ws, hipStream_t stream) {
  return pitch_run(x, lengths, rows, T, srate, 1.0, nullptr, nullptr, nullptr, cmnd, ctot, ws,
                   stream);
}

extern "C" int segan_pitch_frames(int T, int srate) {
  PitchRate pr;
  if (!pitch_rate(srate, &pr) || T < 0 || T > PITCH_MAX_T) {
    segan_set_error("pitch: bad sizes T=%d srate=%d", T, srate);
    return -1;
  }
  return pitch_frames_of(pitch_blocks(T, pr.H, pr.nl));
}

extern "C" int segan_pitch_dims(int rows, int T, int srate, long long* out) {
  PitchRate pr;
  SEGAN_REQUIRE(out, "pitch: NULL pointer");
  SEGAN_REQUIRE(pitch_sizes_ok(rows, T) && pitch_rate(srate, &pr),
                "pitch: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  const long long nb = pitch_blocks(T, pr.H, pr.nl);
  out[0] = pr.H;
  out[1] = pr.tmin;
  out[2] = pr.tmax;
  out[3] = nb;
  out[4] = pitch_frames_of((int)nb);
  out[5] = (long long)rows * nb * 2 * pr.nl;
  return SEGAN_OK;
}

extern "C" int segan_pitch(const float* x, const int* lengths, int rows, int T, int srate,
                           double theta, double* f0, int* lag, double* ap, double* ws,
                           void* stream) {
  PitchRate pr;
  SEGAN_REQUIRE(x && f0 && lag && ap && ws, "pitch: NULL pointer");
  SEGAN_REQUIRE(pitch_sizes_ok(rows, T) && pitch_rate(srate, &pr),
                "pitch: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  SEGAN_REQUIRE(theta > 0.0 && theta <= 1.0, "pitch: the threshold %g is not in (0, 1]", theta);
  return pitch_run(x, lengths, rows, T, srate, theta, f0, lag, ap, nullptr, nullptr, ws,
                   (hipStream_t)stream);
}

extern "C" int segan_pitch_cmnd(const float* x, const int* lengths, int rows, int T, int srate,
                                double* cmnd, double* ws, void* stream) {
  PitchRate pr;
  SEGAN_REQUIRE(x && cmnd && ws, "pitch: NULL pointer");
  SEGAN_REQUIRE(pitch_sizes_ok(rows, T) && pitch_rate(srate, &pr),
                "pitch: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  return pitch_run(x, lengths, rows, T, srate, 1.0, nullptr, nullptr, nullptr, cmnd, nullptr, ws,
                   (hipStream_t)stream);
}

extern "C" int segan_f0_eval(const double* f0_ref, const int* lag_ref, const double* f0_deg,
                             const int* lag_deg, const int* nframes, int rows, int F,
                             double* out4, void* stream) {
  SEGAN_REQUIRE(f0_ref && lag_ref && f0_deg && lag_deg && out4, "f0_eval: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && F >= 0 && F <= PITCH_MAX_T,
                "f0_eval: bad sizes rows=%d frames=%d", rows, F);
  hipLaunchKernelGGL(f0_eval_kernel, dim3(rows), dim3(64), 0, (hipStream_t)stream, f0_ref, lag_ref,
                     f0_deg, lag_deg, nframes, F, out4);
  return segan_check_launch("f0_eval_kernel");
}
