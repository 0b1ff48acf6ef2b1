// The OM-LSA enhancer with IMCRA noise tracking (scripts/omlsa_oracle.py,
// include/segan_omlsa.h): the log-spectral-amplitude gain weighted with the speech-presence
// probability, on a noise spectrum that follows the minima of the smoothed periodogram over a
// window of U V frames.  fp64 on fp32 or fp64 rows, per-row lengths, no atomics, no scratch, every
// sum in an order fixed by the bin, sample or frame index, so a row's result depends neither on T,
// nor on the other rows, nor on what lies past its length.
//
//   denoise_analysis_kernel   segan_stsa.h, without the noise-frame workgroup
//   omlsa_recursion_kernel    one workgroup per row, one thread per bin, a loop over the frames.
//                             The state of a bin (S, Smin, Smact, St, Stmin, Stmact, lbar, P) is in
//                             registers; the two histories of U slots are in LDS, each thread at
//                             its own bin and a slot that is the same for the whole workgroup.
//                             The neighbour bins of the three-tap smoothings go through LDS: s2
//                             before the first barrier of a frame, I s2 and I before the second.
//                             Each buffer is next written behind the other barrier, which every
//                             thread reaches only after it has read, so two barriers a frame are
//                             all.  presence_t by segan_denoise's fixed-order reduction (each wave
//                             its 64 bins in ascending k, then the waves in ascending order) and
//                             rough_t by ballots: the wave sums of frame t are written behind the
//                             second barrier of frame t and read by thread 0 behind the first
//                             barrier of frame t + 1 (a last barrier after the loop), since
//                             nothing in the recursion waits for them.  G S over S in place
//   denoise_synthesis_kernel  segan_stsa.h
#include "segan_stsa.h"
#include "../../include/segan_omlsa.h"

// the oracle rounds every product and every sum on its own
#pragma clang fp contract(off)

#define OM_U SEGAN_OMLSA_U
#define OM_V SEGAN_OMLSA_V

namespace {

// sm3(a)[k] with the Hermitian mirror at both ends, 0 <= k <= F
__device__ __forceinline__ double om_sm3(const double* a, int k, int F) {
  const int lo = k == 0 ? 1 : k - 1, hi = k == F ? F - 1 : k + 1;
  return (0.25 * a[lo] + 0.5 * a[k]) + 0.25 * a[hi];
}

// steps 1 / 3 of one smoothed periodogram: the value f joins s and the running minima; at t = 0
// it fills the U slots hist[j * stride] of the bin as well
__device__ __forceinline__ void om_smooth(bool first, bool active, double f, double& s,
                                          double& smin, double& smact, double* hist, int stride) {
  const double as = 0.9, bs = 1.0 - as;
  if (first) {
    s = smin = smact = f;
    if (active)
      for (int j = 0; j < OM_U; ++j) hist[j * stride] = f;
  } else {
    s = as * s + bs * f;
    smin = fmin(smin, s);
    smact = fmin(smact, s);
  }
}

// step 9 at the end of a block of V frames: slot j takes the block's minimum
__device__ __forceinline__ void om_roll(int j, bool active, double s, double& smin, double& smact,
                                        double* hist, int stride) {
  double m = smact;          // slot j itself
  for (int i = 0; i < OM_U; ++i)
    if (i != j) m = fmin(m, hist[i * stride]);
  if (active) hist[j * stride] = smact;
  smin = m;
  smact = s;
}

// presence [rows][nfmax], rough int[rows][nfmax] and noise [rows][F + 1] may be NULL; frames from
// the row's own count on get NaN and -1, a row without frames NaN in noise.
__global__ __launch_bounds__(384) void omlsa_recursion_kernel(
    const int* __restrict__ lengths, int T, DnRate dr, int nfmax, double2* __restrict__ spec,
    int* __restrict__ nframes, double* __restrict__ presence, int* __restrict__ rough,
    double* __restrict__ noise) {
  __shared__ double hist[2][OM_U][DN_MAX_F + 1];
  __shared__ double ex[3][DN_MAX_F + 1];   // s2; I s2; I
  __shared__ double shp[8];
  __shared__ int shr[8];
  const int r = blockIdx.x, k = threadIdx.x, F = dr.F;
  const int lane = k & 63, wave = k >> 6, nw = blockDim.x >> 6;
  const int L = segan_row_samples(lengths, r, T);
  const int nf = dn_frames(L, dr);
  if (k == 0) nframes[r] = nf;
  for (int t = nf + k; t < nfmax; t += blockDim.x) {
    if (presence) presence[(size_t)r * nfmax + t] = NAN;
    if (rough) rough[(size_t)r * nfmax + t] = -1;
  }
  if (nf == 0) {   // the whole workgroup, before any barrier
    if (noise && k <= F) noise[(size_t)r * (F + 1) + k] = NAN;
    return;
  }
  // the threads past bin F repeat bin 0 on values they only read: they write nothing, add nothing
  // to the sums, and meet every barrier
  const bool active = k <= F;
  const int kk = active ? k : 0;
  const int stride = DN_MAX_F + 1;
  const double ck = (k == 0 || k == F) ? 1.0 : 2.0;
  const double a = 0.92, b1 = 1.0 - a, ad = 0.85, bd = 1.0 - ad;
  const double bmin = 1.66, g0 = 4.6, g1 = 3.0, z0 = 1.67;
  double S = 0.0, Smin = 0.0, Smact = 0.0, St = 0.0, Stmin = 0.0, Stmact = 0.0;
  double lbar = 0.0, P = 0.0;
  double2* sp = spec + (size_t)r * nfmax * (size_t)(F + 1) + kk;
  double* pres = presence ? presence + (size_t)r * nfmax : nullptr;
  int* rgh = rough ? rough + (size_t)r * nfmax : nullptr;
  for (int t = 0; t < nf; ++t) {
    const bool first = t == 0;
    const double2 X = sp[(size_t)t * (F + 1)];
    const double s2 = X.x * X.x + X.y * X.y;
    if (active) ex[0][k] = s2;
    __syncthreads();
    if (k == 0 && t > 0) {   // the wave sums of frame t - 1
      double v = 0.0;
      int c = 0;
      for (int w = 0; w < nw; ++w) {
        v += shp[w];
        c += shr[w];
      }
      if (pres) pres[t - 1] = (v / (double)F) / 2.0;
      if (rgh) rgh[t - 1] = c;
    }
    // 1, 2
    const double Sf = om_sm3(ex[0], kk, F);
    om_smooth(first, active, Sf, S, Smin, Smact, &hist[0][0][kk], stride);
    const double th = bmin * Smin;
    const bool I = (s2 < g0 * th) && (S < z0 * th);
    if (active) {
      ex[1][k] = I ? s2 : 0.0;
      ex[2][k] = I ? 1.0 : 0.0;
    }
    __syncthreads();
    // 3
    const double den = om_sm3(ex[2], kk, F), num = om_sm3(ex[1], kk, F);
    const double Stf = den > 0.0 ? num / den : (first ? Sf : St);
    om_smooth(first, active, Stf, St, Stmin, Stmact, &hist[1][0][kk], stride);
    // 4
    const double tth = bmin * Stmin;
    double q = 0.0;
    if (St < z0 * tth) {
      if (s2 <= tth)
        q = 1.0;
      else if (s2 < g1 * tth)
        q = (g1 - s2 / tth) / (g1 - 1.0);
    }
    // 5
    if (first) lbar = s2;
    const double lam = fmax(1.47 * lbar, 0x1p-100);
    const double gam = fmin(s2 / lam, 40.0);
    const double head = first ? a : (a * P) / lam;
    const double xi = fmax(head + b1 * fmax(gam - 1.0, 0.0), 0.0031622776601683794);
    const double A = xi / (1.0 + xi);
    const double nu = A * gam;
    // 6
    double p;
    if (q == 1.0)
      p = 0.0;
    else if (q == 0.0)
      p = 1.0;
    else
      p = 1.0 / (1.0 + ((q / (1.0 - q)) * (1.0 + xi)) * exp(-nu));
    // 7
    const double at = ad + bd * p;
    lbar = at * lbar + (1.0 - at) * s2;
    // 8
    const double GH1 = A * exp(dn_exp1(fmax(nu, 0x1p-40)) / 2.0);
    const double G = exp(p * log(GH1) + (1.0 - p) * -2.878231366242557);
    P = (GH1 * GH1) * s2;
    if (active) sp[(size_t)t * (F + 1)] = make_double2(G * X.x, G * X.y);
    // 9
    if ((t + 1) % OM_V == 0) {
      const int j = ((t + 1) / OM_V - 1) % OM_U;
      om_roll(j, active, S, Smin, Smact, &hist[0][0][kk], stride);
      om_roll(j, active, St, Stmin, Stmact, &hist[1][0][kk], stride);
    }
    // 10
    const double term = active ? ck * p : 0.0;
    double acc = 0.0;
    for (int i = 0; i < 64; ++i) acc += __shfl(term, i, 64);
    const int cnt = __popcll(__ballot(active && I));
    if (lane == 0) {
      shp[wave] = acc;
      shr[wave] = cnt;
    }
    if (t == nf - 1 && noise && active) noise[(size_t)r * (F + 1) + k] = lam;
  }
  __syncthreads();
  if (k == 0) {
    double v = 0.0;
    int c = 0;
    for (int w = 0; w < nw; ++w) {
      v += shp[w];
      c += shr[w];
    }
    if (pres) pres[nf - 1] = (v / (double)F) / 2.0;
    if (rgh) rgh[nf - 1] = c;
  }
}

// the spectra alone; a row length without a frame still gets its 16 bytes, so the size is never 0
long long om_ws_bytes(int rows, int nfmax, int F) {
  return (long long)rows * (long long)(nfmax > 0 ? nfmax : 1) * (F + 1) * 16;
}

template <typename Tin>
int om_run(const Tin* x, const int* lengths, int rows, int T, int srate, void* y, int y_dtype,
           int* nframes, double* presence, int* rough, double* noise, void* ws, hipStream_t st) {
  DnRate dr;
  dn_rate(srate, &dr);
  const DnTable* tb = dn_table(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const int nfmax = dn_frames(T, dr), F = dr.F;
  double2* spec = (double2*)ws;
  const int threads = round_up(F + 1, 64);
  if (nfmax > 0) {
    // nfmax workgroups a row: the one for the six noise frames is not launched, lam0 not written
    hipLaunchKernelGGL(denoise_analysis_kernel<Tin>, dim3(nfmax, rows), dim3(threads), 0, st, x,
                       lengths, T, dr, nfmax, (const double*)tb->win, (const double2*)tb->tw, spec,
                       (double*)nullptr);
    if (int e = segan_check_launch("denoise_analysis_kernel")) return e;
  }
  hipLaunchKernelGGL(omlsa_recursion_kernel, dim3(rows), dim3(threads), 0, st, lengths, T, dr,
                     nfmax, spec, nframes, presence, rough, noise);
  if (int e = segan_check_launch("omlsa_recursion_kernel")) return e;
  const dim3 grid(ceil_div(T, dr.H), rows), block(round_up(dr.H, 64));
  if (y_dtype == SEGAN_DT_F64)
    hipLaunchKernelGGL((denoise_synthesis_kernel<Tin, double>), grid, block, 0, st, x, lengths, T,
                       dr, nfmax, (const double2*)tb->tw, (const double2*)spec, (double*)y);
  else
    hipLaunchKernelGGL((denoise_synthesis_kernel<Tin, float>), grid, block, 0, st, x, lengths, T,
                       dr, nfmax, (const double2*)tb->tw, (const double2*)spec, (float*)y);
  return segan_check_launch("denoise_synthesis_kernel");
}

}  // namespace

extern "C" int segan_omlsa_dims(int rows, int T, int srate, long long* out) {
  DnRate dr;
  SEGAN_REQUIRE(out, "omlsa: NULL pointer");
  SEGAN_REQUIRE(dn_sizes_ok(rows, T) && dn_rate(srate, &dr),
                "omlsa: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  const int nfmax = dn_frames(T, dr);
  out[0] = dr.F;
  out[1] = dr.H;
  out[2] = dr.N;
  out[3] = nfmax;
  out[4] = om_ws_bytes(rows, nfmax, dr.F);
  return SEGAN_OK;
}

extern "C" int segan_omlsa(const void* x, int x_dtype, const int* lengths, int rows, int T,
                           int srate, void* y, int y_dtype, int* nframes, double* presence,
                           int* rough, double* noise, void* ws, void* stream) {
  DnRate dr;
  SEGAN_REQUIRE(x && y && nframes && ws, "omlsa: NULL pointer");
  SEGAN_REQUIRE(dn_sizes_ok(rows, T) && dn_rate(srate, &dr),
                "omlsa: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  SEGAN_REQUIRE((x_dtype == SEGAN_DT_F32 || x_dtype == SEGAN_DT_F64) &&
                    (y_dtype == SEGAN_DT_F32 || y_dtype == SEGAN_DT_F64),
                "omlsa: x and y are SEGAN_DT_F32 or SEGAN_DT_F64, got %d and %d", x_dtype,
                y_dtype);
  SEGAN_REQUIRE(((uintptr_t)ws & 15) == 0, "omlsa: the workspace is not 16-byte aligned");
  if (x_dtype == SEGAN_DT_F64)
    return om_run((const double*)x, lengths, rows, T, srate, y, y_dtype, nframes, presence, rough,
                  noise, ws, (hipStream_t)stream);
  return om_run((const float*)x, lengths, rows, T, srate, y, y_dtype, nframes, presence, rough,
                noise, ws, (hipStream_t)stream);
}
