// segan_quality.hip — per-frame objective speech-quality measures of the reference's evaluation
// (segan/utils.py): weighted spectral slope (WSS, utils.py:442-596) and log-likelihood ratio
// (LLR, utils.py:598-716).  Both use the SSNR frame geometry (win = round(30 ms), hop win/4,
// segan_ssnr_frames) and the Hann-like window 0.5*(1 - cos(2*pi*k/(win+1))), k = 1..win, and
// compute in fp64 like numpy.  The window, the DFT twiddles and the critical-band table are built
// on the host with the reference's own expressions and uploaded once per (device, srate).
// Below them, on the same frames and tables but with per-row lengths: the frequency-weighted
// segmental SNR and the LPC cepstrum distance, and SI-SDR over whole rows.
#include "segan_signal.h"

#define QW_NCRIT 25
#define QW_THREADS 256

namespace {

struct QualityTables {
  int device, srate, win, skip, nfft, klo, nb;
  double* window;   // [win]
  double2* tw;      // [nfft]: (cos, sin)(2*pi*m/nfft)
  double* crit;     // [QW_NCRIT][nb]: utils.py:472-497 restricted to bins klo .. klo+nb-1
  double* crit_all; // [QW_NCRIT][nfft/2]: the same filters over every bin (fwSNRseg)
};

SeganDeviceTables<QualityTables> g_tables;

// utils.py:448-451 / 600-605: window length and hop (the SSNR ones: segan_ssnr_frames)
void frame_geometry(int srate, int* win, int* skip) {
  *win = (int)__builtin_round(30.0 * srate / 1000.0);
  *skip = *win / 4;
}

int nfft_of(int win) {   // utils.py:455: int(2 ** np.ceil(np.log(2*winlength)/np.log(2)))
  return (int)pow(2.0, ceil(log(2.0 * win) / log(2.0)));
}

// Builds the tables of srate on the host and uploads them to the current device.
bool build_tables(int srate, QualityTables* tp) {
  QualityTables& t = *tp;
  t.srate = srate;
  frame_geometry(srate, &t.win, &t.skip);
  t.nfft = nfft_of(t.win);
  const int half = t.nfft / 2;
  // utils.py:537-538: time = np.linspace(1, win, win) / (win + 1); 0.5 * (1 - cos(2*pi*time))
  std::vector<double> window(t.win);
  for (int k = 0; k < t.win; ++k) {
    const double time = (double)(k + 1) / (double)(t.win + 1);
    window[k] = 0.5 * (1.0 - cos(2.0 * M_PI * time));
  }
  // utils.py:463-497: Gaussian critical-band filters, zeroed below the -30 dB point
  static const double cent_freq[QW_NCRIT] = {
      50., 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38,
      1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04,
      3276.17, 3597.63};
  static const double bandwidth[QW_NCRIT] = {
      70., 70, 70, 70, 70, 70, 70, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
      140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126,
      321.465, 346.136};
  const double max_freq = srate / 2.0;
  const double bw_min = bandwidth[0];
  const double min_factor = exp(-30. / (2 * 2.303));
  std::vector<double> full((size_t)QW_NCRIT * half);
  int lo = half, hi = 0;
  for (int i = 0; i < QW_NCRIT; ++i) {
    const double f0 = floor((cent_freq[i] / max_freq) * half);
    const double bw = (bandwidth[i] / max_freq) * half;
    const double norm_factor = log(bw_min) - log(bandwidth[i]);
    for (int j = 0; j < half; ++j) {
      const double u = (j - f0) / bw;
      const double v = exp(-11 * (u * u) + norm_factor);
      const double w = v > min_factor ? v : 0.0;
      full[(size_t)i * half + j] = w;
      if (w != 0.0) {
        lo = j < lo ? j : lo;
        hi = j + 1 > hi ? j + 1 : hi;
      }
    }
  }
  if (hi <= lo) {
    segan_set_error("quality: no critical band has a non-zero weight at srate %d", srate);
    return false;
  }
  t.klo = lo;
  t.nb = hi - lo;
  std::vector<double> crit((size_t)QW_NCRIT * t.nb);
  for (int i = 0; i < QW_NCRIT; ++i)
    for (int b = 0; b < t.nb; ++b) crit[(size_t)i * t.nb + b] = full[(size_t)i * half + lo + b];

  return segan_upload(&t.window, window, "quality") &&
         segan_upload(&t.tw, segan_twiddles(t.nfft), "quality") &&
         segan_upload(&t.crit, crit, "quality") && segan_upload(&t.crit_all, full, "quality");
}

// Returns the tables of (current device, srate), building and uploading them on first use.
const QualityTables* get_tables(int srate) {
  return g_tables.get(
      "quality", [=](const QualityTables& t) { return t.srate == srate; },
      [=](QualityTables* t) { return build_tables(srate, t); });
}

}  // namespace

// the windowed (clean, processed) frame f of row blockIdx.y as fp64 pairs: fr[k] = (c, p)
__device__ __forceinline__ void load_frame_pair(double2* fr, const float* __restrict__ ref,
                                                const float* __restrict__ deg,
                                                const double* __restrict__ window, int T,
                                                int f, int win, int skip, int t, int nt) {
  const size_t base = (size_t)blockIdx.y * T + (size_t)f * skip;
  for (int k = t; k < win; k += nt) {
    const double w = window[k];
    fr[k] = make_double2((double)ref[base + k] * w, (double)deg[base + k] * w);
  }
}

// ---------------------------------------------------------------------------------
// WSS.  One 256-thread workgroup per (frame, row).  LDS: the windowed pair, the twiddles, the
// power of both spectra over the bins [klo, klo+nb) that some band weighs (a direct fp64 DFT:
// |sum_n x[n] e^{-2 pi i k n / nfft}|^2, the zero padding of np.fft.fft(x, nfft) contributes
// nothing).  Then 50 band energies (one wave each, lanes over bins), and one lane per band for
// dB, slope, nearest peak and weight, summed across the wave.
// ---------------------------------------------------------------------------------
__global__ __launch_bounds__(QW_THREADS) void wss_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, double* __restrict__ dist, int T,
    int nframes, int win, int skip, int nfft, int klo, int nb, const double* __restrict__ window,
    const double2* __restrict__ twg, const double* __restrict__ crit) {
  extern __shared__ double2 qsh[];
  double2* fr = qsh;              // [win]
  double2* tw = fr + win;         // [nfft]
  double2* spec = tw + nfft;      // [nb]: (clean, processed) power
  __shared__ double energy[2][QW_NCRIT];   // dB
  __shared__ double slope[2][QW_NCRIT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int f = blockIdx.x;
  load_frame_pair(fr, ref, deg, window, T, f, win, skip, t, QW_THREADS);
  for (int m = t; m < nfft; m += QW_THREADS) tw[m] = twg[m];
  __syncthreads();

  const int mask = nfft - 1;   // nfft is a power of two
  for (int b = t; b < nb; b += QW_THREADS) {
    const int k = klo + b;
    double cr = 0.0, ci = 0.0, pr = 0.0, pi = 0.0;
    int idx = 0;
    for (int n = 0; n < win; ++n) {
      const double2 x = fr[n];
      const double2 w = tw[idx];
      cr = fma(x.x, w.x, cr);
      ci = fma(x.x, w.y, ci);
      pr = fma(x.y, w.x, pr);
      pi = fma(x.y, w.y, pi);
      idx = (idx + k) & mask;
    }
    spec[b] = make_double2(cr * cr + ci * ci, pr * pr + pi * pi);
  }
  __syncthreads();

  // band energies: (band, signal) pairs over the four waves
  for (int j = wave; j < 2 * QW_NCRIT; j += QW_THREADS / 64) {
    const int band = j % QW_NCRIT, sig = j / QW_NCRIT;
    const double* cw = crit + (size_t)band * nb;
    double e = 0.0;
    for (int b = lane; b < nb; b += 64) e = fma(sig ? spec[b].y : spec[b].x, cw[b], e);
    e = segan_wave_sum(e);
    // 10*log10(max(E, 1e-10)), NaN propagating like np.max
    if (lane == 0) energy[sig][band] = 10.0 * log10(e < 1e-10 ? 1e-10 : e);
  }
  __syncthreads();
  if (wave == 0 && lane < QW_NCRIT - 1) {
    slope[0][lane] = energy[0][lane + 1] - energy[0][lane];
    slope[1][lane] = energy[1][lane + 1] - energy[1][lane];
  }
  __syncthreads();
  if (wave != 0) return;
  const double Kmax = 20.0, Klocmax = 1.0;
  double num = 0.0, den = 0.0;
  if (lane < QW_NCRIT - 1) {
    const int i = lane;
    double W = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double* e = energy[s];
      const double* sl = slope[s];
      // utils.py:541-560, off-by-one of the right search included
      double peak;
      int n = i;
      if (sl[i] > 0) {
        while (n < QW_NCRIT - 1 && sl[n] > 0) ++n;
        peak = e[n - 1];
      } else {
        while (n >= 0 && sl[n] <= 0) --n;
        peak = e[n + 1];
      }
      double dBmax = e[0];   // python max(): first of the largest
      for (int m = 1; m < QW_NCRIT; ++m)
        if (e[m] > dBmax) dBmax = e[m];
      const double wmax = Kmax / (Kmax + dBmax - e[i]);
      const double wloc = Klocmax / (Klocmax + peak - e[i]);
      W += wmax * wloc;
    }
    W = W / 2;
    const double d = slope[0][i] - slope[1][i];
    num = W * (d * d);
    den = W;
  }
  num = segan_wave_sum(num);
  den = segan_wave_sum(den);
  if (lane == 0) dist[(size_t)blockIdx.y * nframes + f] = num / den;
}

// ---------------------------------------------------------------------------------
// LLR.  One wave per (frame, row), four frames per workgroup.  Lags 0..P of both windowed
// frames (lanes over samples, butterfly sums), Levinson-Durbin in fp64 (lpcoeff, utils.py:
// 659-716) in every lane, R and [1, -a] rounded to fp32 as lpcoeff returns them, both quadratic
// forms A toeplitz(R_clean) A^T in fp64 from those, log of the ratio.  R_clean[0] == 0 yields NaN.
// ---------------------------------------------------------------------------------
// levinson_lpc: segan_signal.h (shared with the whisper stage)
template <int P>
__device__ __forceinline__ double quad_toeplitz(const double (&A)[P + 1], const double (&R)[P + 1]) {
  double q = 0.0;
#pragma unroll
  for (int i = 0; i <= P; ++i) {
    double r = 0.0;
#pragma unroll
    for (int j = 0; j <= P; ++j) r += A[j] * R[i > j ? i - j : j - i];
    q += A[i] * r;
  }
  return q;
}

template <int P>
__global__ __launch_bounds__(QW_THREADS) void llr_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, double* __restrict__ dist, int T,
    int nframes, int win, int skip, const double* __restrict__ window) {
  extern __shared__ double2 qsh[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * (QW_THREADS / 64) + wave;
  double2* fr = qsh + (size_t)wave * win;
  if (f < nframes) load_frame_pair(fr, ref, deg, window, T, f, win, skip, lane, 64);
  __syncthreads();
  if (f >= nframes) return;   // whole waves leave; no barrier below

  double Rc[P + 1], Rp[P + 1];
#pragma unroll
  for (int j = 0; j <= P; ++j) Rc[j] = Rp[j] = 0.0;
  for (int n = lane; n < win; n += 64) {
    const double2 x = fr[n];
#pragma unroll
    for (int j = 0; j <= P; ++j) {
      if (n + j < win) {
        const double2 y = fr[n + j];
        Rc[j] = fma(x.x, y.x, Rc[j]);
        Rp[j] = fma(x.y, y.y, Rp[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j <= P; ++j) {
    Rc[j] = segan_wave_sum(Rc[j]);
    Rp[j] = segan_wave_sum(Rp[j]);
  }
  double Ac[P + 1], Ap[P + 1];
  levinson_lpc<P>(Rc, Ac);
  levinson_lpc<P>(Rp, Ap);
  double Rcf[P + 1];
#pragma unroll
  for (int j = 0; j <= P; ++j) Rcf[j] = (double)(float)Rc[j];
  const double numer = quad_toeplitz<P>(Ap, Rcf);
  const double denom = quad_toeplitz<P>(Ac, Rcf);
  if (lane == 0) dist[(size_t)blockIdx.y * nframes + f] = log(numer / denom);
}

static int quality_args(const char* what, const float* ref, const float* deg, const double* dist,
                        int rows, int T, int srate) {
  SEGAN_REQUIRE(ref && deg && dist, "%s: NULL pointer", what);
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && T > 0, "%s: bad sizes rows=%d T=%d", what, rows, T);
  int win, skip;
  frame_geometry(srate > 0 ? srate : 0, &win, &skip);
  // 2*win <= 2048 keeps the frames and twiddles of either kernel within 64 KiB of LDS
  SEGAN_REQUIRE(srate > 0 && skip > 0 && nfft_of(win) <= 2048,
                "%s: srate %d unsupported (30 ms window of 4 .. 1024 samples)", what, srate);
  return SEGAN_OK;
}

extern "C" int segan_wss(const float* ref, const float* deg, double* dist, int rows, int T,
                         int srate, void* stream) {
  if (int e = quality_args("wss", ref, deg, dist, rows, T, srate)) return e;
  const int nf = segan_ssnr_frames(T, srate);
  if (nf == 0) return SEGAN_OK;
  const QualityTables* tb = get_tables(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const size_t lds = (size_t)(tb->win + tb->nfft + tb->nb) * sizeof(double2);
  hipLaunchKernelGGL(wss_kernel, dim3(nf, rows), dim3(QW_THREADS), lds, (hipStream_t)stream, ref,
                     deg, dist, T, nf, tb->win, tb->skip, tb->nfft, tb->klo, tb->nb, tb->window,
                     tb->tw, tb->crit);
  return segan_check_launch("wss_kernel");
}

extern "C" int segan_llr(const float* ref, const float* deg, double* dist, int rows, int T,
                         int srate, void* stream) {
  if (int e = quality_args("llr", ref, deg, dist, rows, T, srate)) return e;
  const int nf = segan_ssnr_frames(T, srate);
  if (nf == 0) return SEGAN_OK;
  const QualityTables* tb = get_tables(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const size_t lds = (size_t)(QW_THREADS / 64) * tb->win * sizeof(double2);
  const dim3 grid(ceil_div(nf, QW_THREADS / 64), rows);
  hipStream_t st = (hipStream_t)stream;
  if (srate >= 10000)   // utils.py:607-611: LPC order
    hipLaunchKernelGGL(llr_kernel<16>, grid, dim3(QW_THREADS), lds, st, ref, deg, dist, T, nf,
                       tb->win, tb->skip, tb->window);
  else
    hipLaunchKernelGGL(llr_kernel<10>, grid, dim3(QW_THREADS), lds, st, ref, deg, dist, T, nf,
                       tb->win, tb->skip, tb->window);
  return segan_check_launch("llr_kernel");
}

// ---------------------------------------------------------------------------------
// Measures with per-row lengths: fwSNRseg and the LPC cepstrum distance on
// the frames above, SI-SDR on whole rows.  Row r is its first lengths[r] samples (clamped to
// [0, T]; NULL: all T) and has segan_ssnr_frames(lengths[r], srate) frames of its own; every
// sum runs in an order fixed by the sample or frame index alone, so a row's result does not
// depend on T, on the other rows or on what lies past its length.
// ---------------------------------------------------------------------------------
__device__ __forceinline__ int row_frames(int L, int win, int skip) {   // segan_ssnr_frames
  const int nf = (int)((double)L / skip - (double)win / skip);
  return nf > 0 ? nf : 0;
}

// fwSNRseg.  WSS's layout: one 256-thread workgroup per (frame, row), the windowed pair and the
// twiddles in LDS, a direct fp64 DFT, here of all nfft/2 bins (at most QF_BINS per thread, kept
// in registers) and to the magnitude.  The block sum of the magnitudes normalises them into the
// first half of the twiddle array, which no DFT reads any more; then 50 band values (one wave
// each, lanes over bins) and one lane per band for weight and SNR.
#define QF_BINS 4   // nfft/2 <= 1024 = QF_BINS * QW_THREADS (quality_args)

__global__ __launch_bounds__(QW_THREADS) void fwsegsnr_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, const int* __restrict__ lengths,
    double* __restrict__ frames_out, int T, int nframes, int win, int skip, int nfft,
    const double* __restrict__ window, const double2* __restrict__ twg,
    const double* __restrict__ crit_all) {
  extern __shared__ double2 qsh[];
  double2* fr = qsh;         // [win]
  double2* tw = fr + win;    // [nfft]; after the DFT [nfft/2]: normalised (clean, processed) magnitude
  __shared__ double wsum[QW_THREADS / 64][2];
  __shared__ double band[2][QW_NCRIT];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int f = blockIdx.x, r = blockIdx.y;
  if (f >= row_frames(segan_row_samples(lengths, r, T), win, skip)) {   // the whole workgroup
    if (t == 0) frames_out[(size_t)r * nframes + f] = NAN;
    return;
  }
  load_frame_pair(fr, ref, deg, window, T, f, win, skip, t, QW_THREADS);
  for (int m = t; m < nfft; m += QW_THREADS) tw[m] = twg[m];
  __syncthreads();

  const int half = nfft >> 1, mask = nfft - 1;   // nfft is a power of two
  double2 mag[QF_BINS];
  double tot[2] = {0.0, 0.0};
#pragma unroll
  for (int i = 0; i < QF_BINS; ++i) {
    const int k = t + i * QW_THREADS;
    mag[i] = make_double2(0.0, 0.0);
    if (k < half) {
      double cr = 0.0, ci = 0.0, pr = 0.0, pi = 0.0;
      int idx = 0;
      for (int n = 0; n < win; ++n) {
        const double2 x = fr[n];
        const double2 w = tw[idx];
        cr = fma(x.x, w.x, cr);
        ci = fma(x.x, w.y, ci);
        pr = fma(x.y, w.x, pr);
        pi = fma(x.y, w.y, pi);
        idx = (idx + k) & mask;
      }
      mag[i] = make_double2(sqrt(cr * cr + ci * ci), sqrt(pr * pr + pi * pi));
    }
    tot[0] += mag[i].x;
    tot[1] += mag[i].y;
  }
  block_sum_fixed<2>(tot, wsum);   // its barrier: every DFT has read its twiddles
#pragma unroll
  for (int i = 0; i < QF_BINS; ++i) {
    const int k = t + i * QW_THREADS;
    if (k < half) tw[k] = make_double2(mag[i].x / tot[0], mag[i].y / tot[1]);   // 0/0: NaN frame
  }
  __syncthreads();

  for (int j = wave; j < 2 * QW_NCRIT; j += QW_THREADS / 64) {
    const int b = j % QW_NCRIT, sig = j / QW_NCRIT;
    const double* cw = crit_all + (size_t)b * half;
    double e = 0.0;
    for (int k = lane; k < half; k += 64) e = fma(sig ? tw[k].y : tw[k].x, cw[k], e);
    e = segan_wave_sum(e);
    if (lane == 0) band[sig][b] = e;
  }
  __syncthreads();
  if (wave != 0) return;
  double num = 0.0, den = 0.0;
  if (lane < QW_NCRIT) {
    const double ce = band[0][lane], d = ce - band[1][lane];
    double err = d * d;
    if (err < 0x1p-52) err = 0x1p-52;   // a NaN stays
    den = pow(ce, 0.2);
    num = den * (10.0 * log10(ce * ce / err));
  }
  num = segan_wave_sum(num);
  den = segan_wave_sum(den);
  const double v = num / den;
  if (lane == 0)
    frames_out[(size_t)r * nframes + f] = isfinite(v) ? (v < -10.0 ? -10.0 : (v > 35.0 ? 35.0 : v))
                                                      : (double)NAN;
}

// row_out[r] = the mean of the row's finite frame values (NaN without any): threads over frames
// in strides of 256, then block_sum_fixed
__global__ __launch_bounds__(QW_THREADS) void fwsegsnr_rows_kernel(
    const double* __restrict__ frames, const int* __restrict__ lengths,
    double* __restrict__ row_out, int T, int nframes, int win, int skip) {
  __shared__ double sh[QW_THREADS / 64][2];
  const int r = blockIdx.x;
  const int nf = row_frames(segan_row_samples(lengths, r, T), win, skip);
  double acc[2] = {0.0, 0.0};
  for (int f = threadIdx.x; f < nf && f < nframes; f += QW_THREADS) {
    const double v = frames[(size_t)r * nframes + f];
    if (v == v) {
      acc[0] += v;
      acc[1] += 1.0;
    }
  }
  block_sum_fixed<2>(acc, sh);
  if (threadIdx.x == 0) row_out[r] = acc[1] > 0.0 ? acc[0] / acc[1] : (double)NAN;
}

// the LPC cepstrum c[1..P] of the prediction polynomial A = [1, a_1 .. a_P]:
// c_1 = -a_1, c_n = -a_n - (1/n) sum_{k=1}^{n-1} k c_k a_{n-k}
template <int P>
__device__ __forceinline__ void lpc_cepstrum(const double (&A)[P + 1], double (&c)[P + 1]) {
  c[0] = 0.0;
  c[1] = -A[1];
#pragma unroll
  for (int n = 2; n <= P; ++n) {
    double s = 0.0;
#pragma unroll
    for (int k = 1; k < n; ++k) s += (double)k * c[k] * A[n - k];
    c[n] = -A[n] - s / (double)n;
  }
}

// Cepstrum distance.  LLR's layout and lags: one wave per (frame, row), four frames per
// workgroup; Levinson-Durbin in fp64 without LLR's fp32 rounding, the cepstra of both frames,
// min(10, 10 sqrt(2) / ln 10 * ||c_clean - c_processed||).  A frame of no energy yields NaN.
template <int P>
__global__ __launch_bounds__(QW_THREADS) void cepdist_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, const int* __restrict__ lengths,
    double* __restrict__ dist, int T, int nframes, int win, int skip,
    const double* __restrict__ window) {
  extern __shared__ double2 qsh[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * (QW_THREADS / 64) + wave, r = blockIdx.y;
  const bool live = f < nframes && f < row_frames(segan_row_samples(lengths, r, T), win, skip);
  double2* fr = qsh + (size_t)wave * win;
  if (live) load_frame_pair(fr, ref, deg, window, T, f, win, skip, lane, 64);
  else if (f < nframes && lane == 0) dist[(size_t)r * nframes + f] = NAN;
  __syncthreads();
  if (!live) return;   // whole waves leave; no barrier below

  double Rc[P + 1], Rp[P + 1];
#pragma unroll
  for (int j = 0; j <= P; ++j) Rc[j] = Rp[j] = 0.0;
  for (int n = lane; n < win; n += 64) {
    const double2 x = fr[n];
#pragma unroll
    for (int j = 0; j <= P; ++j) {
      if (n + j < win) {
        const double2 y = fr[n + j];
        Rc[j] = fma(x.x, y.x, Rc[j]);
        Rp[j] = fma(x.y, y.y, Rp[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j <= P; ++j) {
    Rc[j] = segan_wave_sum(Rc[j]);
    Rp[j] = segan_wave_sum(Rp[j]);
  }
  double A[P + 1], cc[P + 1], cp[P + 1];
  levinson_lpc<P, false>(Rc, A);
  lpc_cepstrum<P>(A, cc);
  levinson_lpc<P, false>(Rp, A);
  lpc_cepstrum<P>(A, cp);
  double d2 = 0.0;
#pragma unroll
  for (int n = 1; n <= P; ++n) d2 += (cc[n] - cp[n]) * (cc[n] - cp[n]);
  const double d = (10.0 * sqrt(2.0) / log(10.0)) * sqrt(d2);
  if (lane == 0)
    dist[(size_t)r * nframes + f] = (Rc[0] == 0.0 || Rp[0] == 0.0) ? (double)NAN
                                                                   : (d > 10.0 ? 10.0 : d);
}

// SI-SDR.  Each row is cut into spans of SEGAN_SISDR_SPAN samples, one workgroup per span (the
// grid comes from T alone; workgroups past a row's length leave).  Pass 1: the span's (sum s,
// sum x, sum s s, sum s x); a wave per row adds the spans in turn and derives both means and
// alpha from the moments (an error d of alpha moves <e, e> by d^2 only: e is orthogonal to s).
// Pass 2: the span's (sum (s - ms)^2, sum e^2) with e = alpha (s - ms) - (x - mx) sample by
// sample; the last kernel adds the spans and takes the ratio.
__global__ __launch_bounds__(QW_THREADS) void sisdr_span_kernel(
    const float* __restrict__ ref, const float* __restrict__ deg, const int* __restrict__ lengths,
    int T, int nspans, const double* __restrict__ stat, double* __restrict__ part) {
  __shared__ double sh[QW_THREADS / 64][4];
  const int r = blockIdx.y;
  const long long L = segan_row_samples(lengths, r, T);
  const long long start = (long long)blockIdx.x * SEGAN_SISDR_SPAN;
  if (start >= L) return;   // the whole workgroup
  const long long end = start + SEGAN_SISDR_SPAN < L ? start + SEGAN_SISDR_SPAN : L;
  const float* s = ref + (size_t)r * T;
  const float* x = deg + (size_t)r * T;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (!stat) {
    for (long long i = start + threadIdx.x; i < end; i += QW_THREADS) {
      const double a = s[i], b = x[i];
      acc[0] += a;
      acc[1] += b;
      acc[2] = fma(a, a, acc[2]);
      acc[3] = fma(a, b, acc[3]);
    }
  } else {
    const double ms = stat[4 * r], mx = stat[4 * r + 1], alpha = stat[4 * r + 2];
    for (long long i = start + threadIdx.x; i < end; i += QW_THREADS) {
      const double a = (double)s[i] - ms, e = alpha * a - ((double)x[i] - mx);
      acc[0] = fma(a, a, acc[0]);
      acc[1] = fma(e, e, acc[1]);
    }
  }
  block_sum_fixed<4>(acc, sh);
  if (threadIdx.x == 0) {
    double* p = part + ((size_t)r * nspans + blockIdx.x) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] = acc[j];
  }
}

// one wave per row: the row's spans added (lanes over spans in strides of 64, then the butterfly);
// row_out == NULL: (mean s, mean x, alpha) into stat; else the SI-SDR into row_out
__global__ __launch_bounds__(64) void sisdr_final_kernel(
    const int* __restrict__ lengths, int T, int nspans, const double* __restrict__ part,
    double* __restrict__ stat, double* __restrict__ row_out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int L = segan_row_samples(lengths, r, T);
  const int mine = (int)(((long long)L + SEGAN_SISDR_SPAN - 1) / SEGAN_SISDR_SPAN);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = lane; b < mine && b < nspans; b += 64) {
    const double* p = part + ((size_t)r * nspans + b) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += p[j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = segan_wave_sum(acc[j]);
  if (lane != 0) return;
  if (!row_out) {
    const double n = (double)L;
    stat[4 * r] = acc[0] / n;
    stat[4 * r + 1] = acc[1] / n;
    stat[4 * r + 2] = (acc[3] - acc[0] * acc[1] / n) / (acc[2] - acc[0] * acc[0] / n);
  } else {
    const double alpha = stat[4 * r + 2], ss = acc[0], ee = acc[1];
    row_out[r] = !(ss > 0.0) ? (double)NAN
                             : (ee == 0.0 ? (double)INFINITY : 10.0 * log10(alpha * alpha * ss / ee));
  }
}

extern "C" int segan_fwsegsnr(const float* ref, const float* deg, const int* lengths, int rows,
                              int T, int srate, double* frames_out, double* row_out, void* stream) {
  if (int e = quality_args("fwsegsnr", ref, deg, frames_out, rows, T, srate)) return e;
  SEGAN_REQUIRE(row_out, "fwsegsnr: NULL pointer");
  const QualityTables* tb = get_tables(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const int nf = segan_ssnr_frames(T, srate);
  hipStream_t st = (hipStream_t)stream;
  if (nf > 0) {
    const size_t lds = (size_t)(tb->win + tb->nfft) * sizeof(double2);
    hipLaunchKernelGGL(fwsegsnr_kernel, dim3(nf, rows), dim3(QW_THREADS), lds, st, ref, deg,
                       lengths, frames_out, T, nf, tb->win, tb->skip, tb->nfft, tb->window, tb->tw,
                       tb->crit_all);
    if (int e = segan_check_launch("fwsegsnr_kernel")) return e;
  }
  hipLaunchKernelGGL(fwsegsnr_rows_kernel, dim3(rows), dim3(QW_THREADS), 0, st, frames_out, lengths,
                     row_out, T, nf, tb->win, tb->skip);
  return segan_check_launch("fwsegsnr_rows_kernel");
}

extern "C" int segan_cepdist(const float* ref, const float* deg, const int* lengths, int rows,
                             int T, int srate, double* frames_out, void* stream) {
  if (int e = quality_args("cepdist", ref, deg, frames_out, rows, T, srate)) return e;
  const int nf = segan_ssnr_frames(T, srate);
  if (nf == 0) return SEGAN_OK;
  const QualityTables* tb = get_tables(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const size_t lds = (size_t)(QW_THREADS / 64) * tb->win * sizeof(double2);
  const dim3 grid(ceil_div(nf, QW_THREADS / 64), rows);
  hipStream_t st = (hipStream_t)stream;
  if (srate >= 10000)
    hipLaunchKernelGGL(cepdist_kernel<16>, grid, dim3(QW_THREADS), lds, st, ref, deg, lengths,
                       frames_out, T, nf, tb->win, tb->skip, tb->window);
  else
    hipLaunchKernelGGL(cepdist_kernel<10>, grid, dim3(QW_THREADS), lds, st, ref, deg, lengths,
                       frames_out, T, nf, tb->win, tb->skip, tb->window);
  return segan_check_launch("cepdist_kernel");
}

extern "C" int segan_sisdr(const float* ref, const float* deg, const int* lengths, int rows, int T,
                           double* row_out, double* ws, void* stream) {
  SEGAN_REQUIRE(ref && deg && row_out && ws, "sisdr: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= 65535 && T > 0, "sisdr: bad sizes rows=%d T=%d", rows, T);
  const int nspans = (int)(((long long)T + SEGAN_SISDR_SPAN - 1) / SEGAN_SISDR_SPAN);
  double* part = ws;                              // [rows][nspans][4]
  double* stat = ws + (size_t)rows * nspans * 4;  // [rows][4]
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nspans, rows);
  hipLaunchKernelGGL(sisdr_span_kernel, grid, dim3(QW_THREADS), 0, st, ref, deg, lengths, T, nspans,
                     (const double*)nullptr, part);
  if (int e = segan_check_launch("sisdr_span_kernel")) return e;
  hipLaunchKernelGGL(sisdr_final_kernel, dim3(rows), dim3(64), 0, st, lengths, T, nspans, part,
                     stat, (double*)nullptr);
  if (int e = segan_check_launch("sisdr_final_kernel")) return e;
  hipLaunchKernelGGL(sisdr_span_kernel, grid, dim3(QW_THREADS), 0, st, ref, deg, lengths, T, nspans,
                     stat, part);
  if (int e = segan_check_launch("sisdr_span_kernel")) return e;
  hipLaunchKernelGGL(sisdr_final_kernel, dim3(rows), dim3(64), 0, st, lengths, T, nspans, part,
                     stat, row_out);
  return segan_check_launch("sisdr_final_kernel");
}
