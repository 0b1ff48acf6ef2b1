// segan_reverb.hip — on-the-fly reverberation: each row of a batch is
// convolved with its own room impulse response by uniformly partitioned overlap-save convolution.
//   y[n] = sum_{k < L} h[k] x[n + d - k],  n = -1 .. len-1,  x[-1] = prev, zero elsewhere
// Partition P = SEGAN_REVERB_P samples, transform size 2P.  The two transforms are segan_gemm
// (exact fp32 MFMA) against a shared basis, as in segan_stft.hip; this file holds the staging of
// the rows, the frequency-domain delay line between the two GEMMs and the output stage.
//
// Spectrum of a real 2P frame, packed into exactly 2P floats (K of the inverse GEMM, no padding):
//   column f,     f = 0 .. P      : Re X[f]
//   column P + f, f = 1 .. P - 1  : Im X[f]        (Im X[0] = Im X[P] = 0 are not stored)
// Row r of a batch owns NB consecutive blocks of P samples of the staging buffer:
//   block 0 = P-1 zeros and prev, blocks 1 .. = x, zero up to and including block NB-1.
// One leading zero block precedes row 0, so frame g = blocks (g, g+1) of the buffer = blocks
// (a-1, a) of row r for g = r NB + a: its alias-free half is block a of the row, and block -1 is
// the all-zero last block of the row before (or the leading block).  The convolution output at
// row position p therefore is element p of the row's NB*P inverse-transformed samples.
#include "segan_signal.h"

#define RV_P SEGAN_REVERB_P
#define RV_N (2 * RV_P)
#define RV_AT 8             // output blocks per thread of the delay line
#define RV_MIN_FRAMES 32    // both GEMMs always take segan_gemm's 128 x 128 path
#define RV_KBLOCK 64        // blocked accumulation of the inverse transform and of the bank's

static_assert(RV_P % 64 == 0 && RV_P <= 1024, "one thread per bin pair, whole waves");

// ---- shared basis: fwd [2P time][2P columns], inv [2P columns][P outputs n = P .. 2P-1] ----
__global__ void reverb_basis_kernel(float* __restrict__ fwd, float* __restrict__ inv) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= RV_N * RV_N) return;
  const int j = idx / RV_N, col = idx - j * RV_N;
  const bool im = col > RV_P;
  const int f = im ? col - RV_P : col;
  double s, c;
  // exact argument reduction in integers, then double precision sincospi
  sincospi(2.0 * (double)((f * j) % RV_N) / (double)RV_N, &s, &c);
  fwd[idx] = (float)(im ? -s : c);
  if (j < RV_P) {
    const int n = RV_P + j;
    sincospi(2.0 * (double)((f * n) % RV_N) / (double)RV_N, &s, &c);
    const double w = (f == 0 || f == RV_P) ? 1.0 : 2.0;
    inv[(size_t)col * RV_P + j] = (float)((im ? -w * s : w * c) / (double)RV_N);
  }
}

// ---- a row's RIR: table[id] = (first partition, partitions, taps, delay) ----
struct RvRow {
  int off, np, d, st;
};

__device__ __forceinline__ RvRow rv_row(const int* __restrict__ ids, const int* __restrict__ table,
                                        int n_rirs, long long bank_parts, int r, int T, int NB) {
  RvRow m = {0, 0, 0, 0};
  const int id = ids[r];
  if (id < 0 || id >= n_rirs) {
    m.st = SEGAN_REVERB_ST_RIR;
    return m;
  }
  const int off = table[4 * id], np = table[4 * id + 1], taps = table[4 * id + 2],
            d = table[4 * id + 3];
  if (off < 0 || np < 1 || (long long)off + np > bank_parts || taps < 1 ||
      (long long)taps > (long long)np * RV_P || d < 0 || d >= taps) {
    m.st = SEGAN_REVERB_ST_RIR;
    return m;
  }
  // the last sample read by the output stage: row position P + T - 1 + d
  if ((long long)RV_P + T - 1 + d > (long long)NB * RV_P - 1) {
    m.st = SEGAN_REVERB_ST_DELAY;
    return m;
  }
  m.off = off;
  m.np = np;
  m.d = d;
  return m;
}

// ---- staging: (frames + 1) blocks of P samples ----
__global__ __launch_bounds__(256) void reverb_stage_kernel(
    const float* __restrict__ x, const int* __restrict__ lengths, const float* __restrict__ prev,
    float* __restrict__ xs, int rows, int T, int NB, size_t total) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total;
       e += (size_t)gridDim.x * blockDim.x) {
    const size_t blk = e / RV_P;
    float v = 0.0f;
    if (blk >= 1) {
      const size_t g = blk - 1;
      const size_t r = g / NB;
      if (r < (size_t)rows) {
        const long long pos = (long long)(g - r * NB) * RV_P + (long long)(e - blk * RV_P);
        const long long n = pos - RV_P;
        if (n == -1)
          v = prev ? prev[r] : 0.0f;
        else if (n >= 0 && n < segan_row_samples(lengths, (int)r, T))
          v = x[r * (size_t)T + n];
      }
    }
    xs[e] = v;
  }
}

// ---- frequency-domain delay line ----
//   Y[r, a, f] = sum_{b < np(r), b <= a} X[r, a-b, f] H[off(r) + b, f]   (complex, b ascending)
// Thread f of a workgroup owns bin f (thread 0: the two real bins 0 and P) for RV_AT consecutive
// output blocks a0 .. a0+AT-1: H[b] is loaded once per b for AT products, and X[a-b] slides
// through a register window of AT frames (one new frame per b), so each X is loaded once per
// workgroup instead of AT times.  The reuse is along a and b at a fixed f, i.e. inside a lane:
// registers carry it and LDS would add nothing.  Lanes run along f: every load and store is a
// contiguous 4 P byte segment.  No atomics, no scratch; a row's result depends on nothing but its
// own frames and RIR.
__global__ __launch_bounds__(RV_P) void reverb_fdl_kernel(
    const float* __restrict__ X, const float* __restrict__ H, const int* __restrict__ ids,
    const int* __restrict__ table, int n_rirs, long long bank_parts, float* __restrict__ Y,
    int rows, int T, int NB, int frames) {
  const int r = blockIdx.y, f = threadIdx.x;
  if (r >= rows) {   // the frames that only pad the GEMMs' M
    for (int g = rows * NB + blockIdx.x; g < frames; g += gridDim.x) {
      Y[(size_t)g * RV_N + f] = 0.0f;
      Y[(size_t)g * RV_N + RV_P + f] = 0.0f;
    }
    return;
  }
  const int a0 = blockIdx.x * RV_AT;
  const RvRow m = rv_row(ids, table, n_rirs, bank_parts, r, T, NB);
  const float* Xr = X + (size_t)r * NB * RV_N;
  const float* Hr = H + (size_t)m.off * RV_N;
  int bend = a0 + RV_AT < NB ? a0 + RV_AT : NB;   // b <= a <= min(a0 + AT, NB) - 1
  if (m.np < bend) bend = m.np;                   // a flagged row has np = 0 and reads nothing
  const bool cplx = f != 0;
  float wr[RV_AT], wi[RV_AT], ar[RV_AT], ai[RV_AT];
#pragma unroll
  for (int j = 0; j < RV_AT; ++j) {
    ar[j] = ai[j] = 0.0f;
    wr[j] = wi[j] = 0.0f;
    if (j > 0 && a0 + j < NB && bend > 0) {
      wr[j] = Xr[(size_t)(a0 + j) * RV_N + f];
      wi[j] = Xr[(size_t)(a0 + j) * RV_N + RV_P + f];
    }
  }
  // the window holds X[a0 - bc + k], -AT < k < AT, in slot k mod AT
  for (int bc = 0; bc < bend; bc += RV_AT) {
#pragma unroll
    for (int u = 0; u < RV_AT; ++u) {
      const int b = bc + u;
      if (b < bend) {
        const int c = a0 - b, slot = (RV_AT - u) % RV_AT;
        wr[slot] = c >= 0 ? Xr[(size_t)c * RV_N + f] : 0.0f;
        wi[slot] = c >= 0 ? Xr[(size_t)c * RV_N + RV_P + f] : 0.0f;
        const float hr = Hr[(size_t)b * RV_N + f], hi = Hr[(size_t)b * RV_N + RV_P + f];
        // bins 1 .. P-1: (xr + i xi)(hr + i hi); thread 0: two real products xr hr and xi hi
        // (thread 0 still issues the two cross products with a zero factor: a non-finite sample
        // in x, which nothing checks, then reaches both of its bins; the bank's taps are finite)
        const float h_ri = cplx ? -hi : 0.0f, h_ir = cplx ? hi : 0.0f, h_ii = cplx ? hr : hi;
#pragma unroll
        for (int j = 0; j < RV_AT; ++j) {
          const int s = (j - u + RV_AT) % RV_AT;
          ar[j] = fmaf(wr[s], hr, ar[j]);
          ar[j] = fmaf(wi[s], h_ri, ar[j]);
          ai[j] = fmaf(wr[s], h_ir, ai[j]);
          ai[j] = fmaf(wi[s], h_ii, ai[j]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < RV_AT; ++j)
    if (a0 + j < NB) {
      float* y = Y + ((size_t)r * NB + a0 + j) * RV_N;
      y[f] = ar[j];
      y[RV_P + f] = ai[j];
    }
}

// ---- output stage: y[r][n] = yt[r][P + n + d], prev_out[r] = yt[r][P - 1 + d], status ----
__global__ __launch_bounds__(256) void reverb_finish_kernel(
    const float* __restrict__ yt, const float* __restrict__ x, const int* __restrict__ lengths,
    const float* __restrict__ prev, const int* __restrict__ ids, const int* __restrict__ table,
    int n_rirs, long long bank_parts, float* __restrict__ y, float* __restrict__ prev_out,
    int* __restrict__ status, int T, int NB) {
  const int r = blockIdx.y;
  const RvRow m = rv_row(ids, table, n_rirs, bank_parts, r, T, NB);
  const int L = segan_row_samples(lengths, r, T);
  const float* base = yt + (size_t)r * NB * RV_P + RV_P + m.d;
  const float* xr = x + (size_t)r * T;
  float* out = y + (size_t)r * T;
  for (int i = blockIdx.x * 256 + threadIdx.x; i <= T; i += gridDim.x * 256) {
    if (i == T) {
      status[r] = m.st;
      if (prev_out) prev_out[r] = m.st ? (prev ? prev[r] : 0.0f) : base[-1];
    } else if (m.st) {
      out[i] = xr[i];     // a flagged row: y = x, nothing of the bank or the transforms is read
    } else {
      out[i] = i < L ? base[i] : 0.0f;
    }
  }
}

// ---- host side ----
static int rv_blocks(int T, int max_delay) {
  const long long last = (long long)RV_P + T - 1;          // row position of x[T-1]
  long long nb = (last + max_delay) / RV_P + 1;
  if (nb < last / RV_P + 2) nb = last / RV_P + 2;          // one all-zero block ends every row
  return nb > 0x7fffffff ? -1 : (int)nb;
}

extern "C" int segan_reverb_dims(int rows, int T, int max_delay, int max_taps, int64_t* dims) {
  SEGAN_REQUIRE(dims, "reverb_dims: NULL pointer");
  SEGAN_REQUIRE(rows > 0 && rows <= SEGAN_REVERB_MAX_ROWS && T > 0 && T <= (1 << 30) && max_delay >= 0 &&
                    max_taps > max_delay && max_taps <= (1 << 30),
                "reverb_dims: bad sizes rows=%d T=%d max_delay=%d max_taps=%d", rows, T, max_delay,
                max_taps);
  const int NB = rv_blocks(T, max_delay);
  const long long frames = (long long)rows * NB < RV_MIN_FRAMES ? RV_MIN_FRAMES : (long long)rows * NB;
  SEGAN_REQUIRE(NB > 0 && frames <= SEGAN_REVERB_MAX_FRAMES, "reverb_dims: rows=%d T=%d is too large", rows, T);
  dims[0] = RV_P;
  dims[1] = NB;
  dims[2] = frames;
  dims[3] = ceil_div(max_taps, RV_P);
  dims[4] = (frames + 1) * RV_P;      // staging floats
  dims[5] = frames * RV_N;            // floats of X, and of Y
  dims[6] = frames * RV_P;            // floats of the inverse transform
  dims[7] = dims[4] + 2 * dims[5] + dims[6];   // the whole workspace of segan_reverb_rows
  return SEGAN_OK;
}

extern "C" int segan_reverb_basis(float* fwd, float* inv, void* stream) {
  SEGAN_REQUIRE(fwd && inv, "reverb_basis: NULL pointer");
  hipLaunchKernelGGL(reverb_basis_kernel, dim3(ceil_div(RV_N * RV_N, 256)), dim3(256), 0,
                     (hipStream_t)stream, fwd, inv);
  return segan_check_launch("reverb_basis");
}

// C = A B with the contraction in blocks of RV_KBLOCK, each an unsplit segan_gemm added into C
// (SEGAN_GEMM_DETERMINISTIC without scratch: an element depends only on its own row of A).  One
// MFMA accumulator over all 2P terms of an inverse transform carries partial sums far larger than
// the result; blocked, the error against fp64 is half.
static int rv_gemm_blocked(const float* A, int64_t lda, const float* B, int64_t ldb, float* C,
                           int M, int N, int K, int kblock, void* stream) {
  for (int k0 = 0; k0 < K; k0 += kblock) {
    const int kc = K - k0 < kblock ? K - k0 : kblock;
    if (int e = segan_gemm(A + k0, lda, 1, B + (size_t)k0 * ldb, ldb, 1, C, N, M, N, kc,
                           k0 == 0 ? 1 : 0, SEGAN_GEMM_DETERMINISTIC, nullptr, 0, stream))
      return e;
  }
  return SEGAN_OK;
}

// H[n_parts][2P] = spectra of the partitions [taps[b P .. b P + P), P zeros]: the zero half drops
// out of the contraction, so K = P over the basis' first P rows
extern "C" int segan_reverb_bank(const float* taps, int64_t n_parts, const float* fwd, float* H,
                                 void* stream) {
  SEGAN_REQUIRE(taps && fwd && H, "reverb_bank: NULL pointer");
  SEGAN_REQUIRE(n_parts > 0 && n_parts <= 0x7fffffff / RV_N, "reverb_bank: bad partition count %lld",
                (long long)n_parts);
  return rv_gemm_blocked(taps, RV_P, fwd, RV_N, H, (int)n_parts, RV_N, RV_P, RV_KBLOCK, stream);
}

// X [frames][2P] = the overlapping 2P frames at hop P of xs (a strided A operand, no framing pass)
// against fwd; yt [frames][P] = Y against inv
extern "C" int segan_reverb_forward(const float* xs, const float* fwd, float* X, int frames,
                                    void* stream) {
  SEGAN_REQUIRE(xs && fwd && X, "reverb_forward: NULL pointer");
  SEGAN_REQUIRE(frames >= RV_MIN_FRAMES && frames <= SEGAN_REVERB_MAX_FRAMES,
                "reverb_forward: bad frame count %d", frames);
  return rv_gemm_blocked(xs, RV_P, fwd, RV_N, X, frames, RV_N, RV_N, RV_N, stream);
}

extern "C" int segan_reverb_inverse(const float* Y, const float* inv, float* yt, int frames,
                                    void* stream) {
  SEGAN_REQUIRE(Y && inv && yt, "reverb_inverse: NULL pointer");
  SEGAN_REQUIRE(frames >= RV_MIN_FRAMES && frames <= SEGAN_REVERB_MAX_FRAMES,
                "reverb_inverse: bad frame count %d", frames);
  return rv_gemm_blocked(Y, RV_N, inv, RV_P, yt, frames, RV_P, RV_N, RV_KBLOCK, stream);
}

static int rv_check(const char* what, int rows, int T, int NB, int frames) {
  SEGAN_REQUIRE(rows > 0 && rows <= SEGAN_REVERB_MAX_ROWS && T > 0 && T <= (1 << 30), "%s: bad sizes rows=%d T=%d",
                what, rows, T);
  SEGAN_REQUIRE(NB >= rv_blocks(T, 0) && (long long)rows * NB <= frames && frames >= RV_MIN_FRAMES &&
                    frames <= SEGAN_REVERB_MAX_FRAMES,
                "%s: blocks=%d frames=%d do not fit rows=%d T=%d (segan_reverb_dims)", what, NB,
                frames, rows, T);
  return SEGAN_OK;
}

extern "C" int segan_reverb_stage(const float* x, const int* lengths, const float* prev, float* xs,
                                  int rows, int T, int blocks, int frames, void* stream) {
  SEGAN_REQUIRE(x && xs, "reverb_stage: NULL pointer");
  if (int e = rv_check("reverb_stage", rows, T, blocks, frames)) return e;
  const size_t total = ((size_t)frames + 1) * RV_P;
  const int grid = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  hipLaunchKernelGGL(reverb_stage_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, lengths,
                     prev, xs, rows, T, blocks, total);
  return segan_check_launch("reverb_stage");
}

extern "C" int segan_reverb_fdl(const float* X, const float* H, int64_t bank_parts,
                                const int* rir_ids, const int* table, int n_rirs, float* Y,
                                int rows, int T, int blocks, int frames, void* stream) {
  SEGAN_REQUIRE(X && H && rir_ids && table && Y, "reverb_fdl: NULL pointer");
  SEGAN_REQUIRE(bank_parts > 0 && n_rirs > 0, "reverb_fdl: empty bank");
  if (int e = rv_check("reverb_fdl", rows, T, blocks, frames)) return e;
  const int pad = frames > rows * blocks ? 1 : 0;
  hipLaunchKernelGGL(reverb_fdl_kernel, dim3(ceil_div(blocks, RV_AT), rows + pad), dim3(RV_P), 0,
                     (hipStream_t)stream, X, H, rir_ids, table, n_rirs, (long long)bank_parts, Y,
                     rows, T, blocks, frames);
  return segan_check_launch("reverb_fdl");
}

extern "C" int segan_reverb_finish(const float* yt, const float* x, const int* lengths,
                                   const float* prev, int64_t bank_parts, const int* rir_ids,
                                   const int* table, int n_rirs, float* y, float* prev_out,
                                   int* status, int rows, int T, int blocks, int frames,
                                   void* stream) {
  SEGAN_REQUIRE(yt && x && rir_ids && table && y && status, "reverb_finish: NULL pointer");
  SEGAN_REQUIRE(bank_parts > 0 && n_rirs > 0, "reverb_finish: empty bank");
  if (int e = rv_check("reverb_finish", rows, T, blocks, frames)) return e;
  const int bx = ceil_div(T + 1, 256) > 64 ? 64 : ceil_div(T + 1, 256);
  hipLaunchKernelGGL(reverb_finish_kernel, dim3(bx, rows), dim3(256), 0, (hipStream_t)stream, yt, x,
                     lengths, prev, rir_ids, table, n_rirs, (long long)bank_parts, y, prev_out,
                     status, T, blocks);
  return segan_check_launch("reverb_finish");
}

extern "C" int segan_reverb_rows(const float* x, const int* lengths, const float* prev,
                                 const float* H, int64_t bank_parts, const int* rir_ids,
                                 const int* table, int n_rirs, const float* fwd, const float* inv,
                                 int rows, int T, int max_delay, float* ws, int64_t ws_floats,
                                 float* y, float* prev_out, int* status, void* stream) {
  SEGAN_REQUIRE(fwd && inv && ws, "reverb_rows: NULL pointer");
  int64_t dims[8];
  if (int e = segan_reverb_dims(rows, T, max_delay, max_delay + 1, dims)) return e;
  SEGAN_REQUIRE(ws_floats >= dims[7] && ((uintptr_t)ws & 15) == 0,
                "reverb_rows: the workspace needs %lld floats, 16-byte aligned (got %lld)",
                (long long)dims[7], (long long)ws_floats);
  const int NB = (int)dims[1], frames = (int)dims[2];
  float* xs = ws;
  float* X = xs + dims[4];
  float* Y = X + dims[5];
  float* yt = Y + dims[5];
  if (int e = segan_reverb_stage(x, lengths, prev, xs, rows, T, NB, frames, stream)) return e;
  if (int e = segan_reverb_forward(xs, fwd, X, frames, stream)) return e;
  if (int e = segan_reverb_fdl(X, H, bank_parts, rir_ids, table, n_rirs, Y, rows, T, NB, frames,
                               stream))
    return e;
  if (int e = segan_reverb_inverse(Y, inv, yt, frames, stream)) return e;
  return segan_reverb_finish(yt, x, lengths, prev, bank_parts, rir_ids, table, n_rirs, y, prev_out,
                             status, rows, T, NB, frames, stream);
}
