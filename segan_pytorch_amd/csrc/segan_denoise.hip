// The Wiener and log-MMSE baseline enhancers (scripts/denoise_oracle.py): one
// short-time spectral enhancer with two gain rules on the decision-directed a-priori SNR and a
// VAD-gated noise estimate.  fp64 on fp32 or fp64 rows, per-row lengths, no atomics, no scratch,
// every sum in an order fixed by the bin, sample or frame index, so a row's result depends neither
// on T, nor on the other rows, nor on what lies past its length.
//
//   denoise_analysis_kernel   one workgroup per (frame, row) and one more per row for the six
//                             noise frames, one thread per bin: the windowed frame and the N
//                             twiddles in LDS, a direct DFT of the bins 0 .. F in ascending n into
//                             spec [rows][nfmax][F + 1]; the noise workgroup adds |X_j| in ascending
//                             j and writes lambda_0 [rows][F + 1]
//   denoise_recursion_kernel  one workgroup per row, one thread per bin, a loop over the frames
//                             with lambda and P in registers; v_t by a fixed-order reduction (each
//                             wave its 64 bins in ascending k, then the waves in ascending order:
//                             the oracle's groups of 64); G S over S in place
//   denoise_synthesis_kernel  one workgroup per (hop, row), one thread per sample: the inverse DFT
//                             of the two frames that cover the hop at the hop's samples only, the
//                             earlier frame added first; zeros from (nf + 1) H on; a row without
//                             frames is copied
//
// Analysis, synthesis, the tables and E1 are in segan_stsa.h, shared with segan_omlsa.hip.
#include "segan_stsa.h"

// the oracle rounds every product and every sum on its own
#pragma clang fp contract(off)

namespace {

// vad [rows][nfmax] and update int[rows][nfmax] may be NULL; frames from the row's own count on
// get NaN and -1.
__global__ __launch_bounds__(384) void denoise_recursion_kernel(
    const int* __restrict__ lengths, int T, DnRate dr, int nfmax, int rule,
    double2* __restrict__ spec, const double* __restrict__ lam0, int* __restrict__ nframes,
    double* __restrict__ vad, int* __restrict__ update) {
  __shared__ double sh[2][8];
  const int r = blockIdx.x, k = threadIdx.x, F = dr.F;
  const int lane = k & 63, wave = k >> 6, nw = blockDim.x >> 6;
  const int L = segan_row_samples(lengths, r, T);
  const int nf = dn_frames(L, dr);
  if (k == 0) nframes[r] = nf;
  for (int t = nf + k; t < nfmax; t += blockDim.x) {
    if (vad) vad[(size_t)r * nfmax + t] = NAN;
    if (update) update[(size_t)r * nfmax + t] = -1;
  }
  if (nf == 0) return;   // the whole workgroup, before any barrier
  const bool active = k <= F;
  const double ck = (k == 0 || k == F) ? 1.0 : 2.0;
  const double a = 0.98, b1 = 1.0 - a;
  double lam = active ? lam0[(size_t)r * (F + 1) + k] : 1.0;
  double P = 0.0;
  double2* sp = spec + (size_t)r * nfmax * (size_t)(F + 1) + (active ? k : 0);
  for (int t = 0; t < nf; ++t) {
    const double2 S = active ? sp[(size_t)t * (F + 1)] : make_double2(0.0, 0.0);
    const double s2 = S.x * S.x + S.y * S.y;
    const double gam = fmin(s2 / lam, 40.0);
    const double first = t == 0 ? a : a * P / lam;
    const double xi = fmax(first + b1 * fmax(gam - 1.0, 0.0), 0.0031622776601683794);
    const double l = gam * xi / (1.0 + xi) - log(1.0 + xi);
    const double term = active ? ck * l : 0.0;
    double acc = 0.0;
    for (int i = 0; i < 64; ++i) acc += __shfl(term, i, 64);
    if (lane == 0) sh[t & 1][wave] = acc;
    __syncthreads();   // the buffer of frame t - 2 was read before the barrier of frame t - 1
    double v = 0.0;
    for (int w = 0; w < nw; ++w) v += sh[t & 1][w];
    v = v / (double)F;
    const bool upd = v < 0.15;
    if (upd) lam = fmax(0.98 * lam + 0.02 * s2, 0x1p-100);
    const double A = xi / (1.0 + xi);
    double G = A;
    if (rule == SEGAN_DENOISE_LOGMMSE) G = A * exp(0.5 * dn_exp1(fmax(A * gam, 0x1p-40)));
    P = (G * G) * s2;
    if (active) sp[(size_t)t * (F + 1)] = make_double2(G * S.x, G * S.y);
    if (k == 0) {
      if (vad) vad[(size_t)r * nfmax + t] = v;
      if (update) update[(size_t)r * nfmax + t] = upd ? 1 : 0;
    }
  }
}

long long dn_ws_bytes(int rows, int nfmax, int F) {
  return (long long)rows * ((long long)nfmax * (F + 1) * 16 + (long long)(F + 1) * 8);
}

template <typename Tin>
int dn_run(const Tin* x, const int* lengths, int rows, int T, int srate, int rule, void* y,
           int y_dtype, int* nframes, double* vad, int* update, void* ws, hipStream_t st) {
  DnRate dr;
  dn_rate(srate, &dr);
  const DnTable* tb = dn_table(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const int nfmax = dn_frames(T, dr), F = dr.F;
  double2* spec = (double2*)ws;
  double* lam0 = (double*)(spec + (size_t)rows * nfmax * (size_t)(F + 1));
  const int threads = round_up(F + 1, 64);
  if (nfmax > 0) {
    hipLaunchKernelGGL(denoise_analysis_kernel<Tin>, dim3(nfmax + 1, rows), dim3(threads), 0, st,
                       x, lengths, T, dr, nfmax, (const double*)tb->win, (const double2*)tb->tw,
                       spec, lam0);
    if (int e = segan_check_launch("denoise_analysis_kernel")) return e;
  }
  hipLaunchKernelGGL(denoise_recursion_kernel, dim3(rows), dim3(threads), 0, st, lengths, T, dr,
                     nfmax, rule, spec, (const double*)lam0, nframes, vad, update);
  if (int e = segan_check_launch("denoise_recursion_kernel")) return e;
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

extern "C" int segan_denoise_dims(int rows, int T, int srate, long long* out) {
  DnRate dr;
  SEGAN_REQUIRE(out, "denoise: NULL pointer");
  SEGAN_REQUIRE(dn_sizes_ok(rows, T) && dn_rate(srate, &dr),
                "denoise: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  const int nfmax = dn_frames(T, dr);
  out[0] = dr.F;
  out[1] = dr.H;
  out[2] = dr.N;
  out[3] = nfmax;
  out[4] = dn_ws_bytes(rows, nfmax, dr.F);
  return SEGAN_OK;
}

extern "C" int segan_denoise(const void* x, int x_dtype, const int* lengths, int rows, int T,
                             int srate, int rule, void* y, int y_dtype, int* nframes, double* vad,
                             int* update, void* ws, void* stream) {
  DnRate dr;
  SEGAN_REQUIRE(x && y && nframes && ws, "denoise: NULL pointer");
  SEGAN_REQUIRE(dn_sizes_ok(rows, T) && dn_rate(srate, &dr),
                "denoise: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  SEGAN_REQUIRE(rule == SEGAN_DENOISE_WIENER || rule == SEGAN_DENOISE_LOGMMSE,
                "denoise: the rule %d is neither SEGAN_DENOISE_WIENER nor SEGAN_DENOISE_LOGMMSE",
                rule);
  SEGAN_REQUIRE((x_dtype == SEGAN_DT_F32 || x_dtype == SEGAN_DT_F64) &&
                    (y_dtype == SEGAN_DT_F32 || y_dtype == SEGAN_DT_F64),
                "denoise: x and y are SEGAN_DT_F32 or SEGAN_DT_F64, got %d and %d", x_dtype,
                y_dtype);
  SEGAN_REQUIRE(((uintptr_t)ws & 15) == 0, "denoise: the workspace is not 16-byte aligned");
  if (x_dtype == SEGAN_DT_F64)
    return dn_run((const double*)x, lengths, rows, T, srate, rule, y, y_dtype, nframes, vad,
                  update, ws, (hipStream_t)stream);
  return dn_run((const float*)x, lengths, rows, T, srate, rule, y, y_dtype, nframes, vad, update,
                ws, (hipStream_t)stream);
}
