// Room impulse responses of shoebox rooms by the image-source method (DESIGN.md section 24,
// scripts/rir_oracle.py, include/segan_rir.h): Allen & Berkley's images with Peterson's
// Hann-windowed sinc of 2 Hw taps for the fractional delays.  fp64, per-row lengths, no atomics,
// no scratch; the sample a thread owns is summed in the order of the image indices, so its bits
// depend neither on count, nor on the other rows, nor on T, nor on lengths beyond the masking.
//
//   rir_kernel        one workgroup per (tile of 256 samples, response), thread j owns sample
//                     t0 + j in a register: a gather, nothing is scattered.  The workgroup walks
//                     the (x image, y image) columns in ascending order, 256 columns at a time,
//                     one per thread.  For a column, rho^2 = px^2 + py^2, and the images that can
//                     reach the tile have pz^2 in [dlo^2 - rho^2, dhi^2 - rho^2]: for k = 0 and 1 a
//                     run of consecutive m below zero and one above, each taken one wider than
//                     computed and kept disjoint.  A prefix sum over the columns' candidate counts
//                     numbers the candidates in enumeration order; they are then taken 256 at a
//                     time, one per thread: tau by the one formula of the oracle, floor, and the
//                     test whether the image touches the tile at all.  Those that do are compacted
//                     by ballots and a sum over the four waves (no LDS append), which keeps the
//                     enumeration order, and every thread sweeps the list: its own test
//                     |k' - f| < Hw decides, so the width of the runs cannot change a bit.  Per
//                     image one sqrt, one sin(pi f) and one sin / cos of pi f / Hw; per tap the
//                     window by the angle-addition identity from the table of (cos, sin)(pi k' /
//                     Hw), and one division.
//                     An image is counted by the tile that holds the first sample it reaches.
//   rir_count_kernel  the tiles' counts of a row added up
#include "segan_signal.h"
#include "../../include/segan_rir.h"

// the oracle rounds every product and every sum on its own
#pragma clang fp contract(off)

#define RIR_TILE SEGAN_RIR_TILE
#define RIR_MAX_HW 64
#define RIR_C 343.0

namespace {

struct RirTable {
  int device, srate;
  double2* cs;   // [2 Hw]: (cos, sin)(pi k' / Hw), k' = -Hw + 1 .. Hw
};
SeganDeviceTables<RirTable> g_rir_tables;

inline bool rir_rate(int srate, int* Hw) {
  if (srate != 16000 && srate != 8000) return false;
  *Hw = srate / 250;
  return true;
}

const RirTable* rir_table(int srate) {
  return g_rir_tables.get(
      "rir", [srate](const RirTable& e) { return e.srate == srate; },
      [srate](RirTable* e) {
        int Hw = 0;
        rir_rate(srate, &Hw);
        std::vector<double2> cs(2 * Hw);
        for (int i = 0; i < 2 * Hw; ++i) {
          const double ang = M_PI * (double)(i - Hw + 1) / (double)Hw;
          cs[i] = make_double2(cos(ang), sin(ang));
        }
        e->srate = srate;
        return segan_upload(&e->cs, cs, "rir");
      });
}

// entries per wall of the power tables: the largest |n - q| of any tile of a row of T samples in a
// room of 1 m, the smallest allowed (the kernel clamps its ranges to it)
inline int rir_stride(int T, int Hw, double rate) {
  const double dhi = (double)(round_up(T, RIR_TILE) + Hw + 1) / rate;
  return (int)floor(dhi / 2.0) + 4;
}

__device__ __forceinline__ int rir_floor(double v) { return (int)floor(v); }

__global__ __launch_bounds__(RIR_TILE) void rir_kernel(
    const double* __restrict__ geom, const double* __restrict__ tables, int stride,
    const int* __restrict__ lengths, int T, int Hw, double rate, const double2* __restrict__ csg,
    double* __restrict__ h, long long* __restrict__ tilecount) {
  __shared__ double2 cs[2 * RIR_MAX_HW];
  __shared__ double c_rho2[RIR_TILE], c_axy[RIR_TILE];
  __shared__ int c_m0[RIR_TILE][4], c_cn[RIR_TILE][4], c_pre[RIR_TILE];
  __shared__ int wsum[4], wacc[4];
  __shared__ long long wcnt[4];
  __shared__ int l_n0[RIR_TILE];
  __shared__ double l_f[RIR_TILE], l_a[RIR_TILE], l_sp[RIR_TILE], l_cf[RIR_TILE], l_sf[RIR_TILE];
  const int r = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x, j = threadIdx.x;
  const int lane = j & 63, wave = j >> 6;
  const int t0 = tile * RIR_TILE, t = t0 + j;
  const int len = segan_row_samples(lengths, r, T);
  double* hr = h + (size_t)r * T;
  if (t0 >= len) {   // the whole workgroup, before any barrier
    if (t < T) hr[t] = 0.0;
    if (tilecount && j == 0) tilecount[(size_t)r * tiles + tile] = 0;
    return;
  }
  const int tend = t0 + RIR_TILE < len ? t0 + RIR_TILE : len;
  for (int i = j; i < 2 * Hw; i += RIR_TILE) cs[i] = csg[i];
  const double* g = geom + (size_t)r * SEGAN_RIR_GEOM;
  const double Lx = g[0], Ly = g[1], Lz = g[2], sx = g[3], sy = g[4], sz = g[5];
  const double rx = g[6], ry = g[7], rz = g[8];
  const double* tb = tables + (size_t)r * 6 * stride;
  // the images that reach the tile have tend + Hw > tau >= t0 - Hw; one sample wider
  const double dhi = (double)(tend + Hw + 1) / rate;
  const double dlo = t0 - Hw - 1 > 0 ? (double)(t0 - Hw - 1) / rate : 0.0;
  const double dhi2 = dhi * dhi, dlo2 = dlo * dlo;
  const int lim = stride - 2;   // |n|, |l|, |m| stay below: |n - q| <= stride - 1
  int Nx = rir_floor(dhi / (2.0 * Lx)) + 2, Ny = rir_floor(dhi / (2.0 * Ly)) + 2;
  Nx = Nx < lim ? Nx : lim;
  Ny = Ny < lim ? Ny : lim;
  const int NYt = 2 * (2 * Ny + 1);
  const long long ncols = (long long)(2 * (2 * Nx + 1)) * NYt;
  const double twoLz = 2.0 * Lz;
  double acc = 0.0;
  long long cnt = 0;
  for (long long c0 = 0; c0 < ncols; c0 += RIR_TILE) {
    const long long c = c0 + j;
    int m0[4] = {0, 0, 0, 0}, cn[4] = {0, 0, 0, 0};
    double rho2 = 0.0, axy = 0.0;
    if (c < ncols) {
      const int ix = (int)(c / NYt), iy = (int)(c - (long long)ix * NYt);
      const int n = (ix >> 1) - Nx, q = ix & 1, l = (iy >> 1) - Ny, jj = iy & 1;
      const double px = ((q ? -sx : sx) - rx) + (double)(2 * n) * Lx;
      const double py = ((jj ? -sy : sy) - ry) + (double)(2 * l) * Ly;
      rho2 = px * px + py * py;
      const double zhi2 = dhi2 - rho2;
      if (zhi2 >= 0.0) {
        axy = (tb[abs(n - q)] * tb[stride + abs(n)]) *
              (tb[2 * stride + abs(l - jj)] * tb[3 * stride + abs(l)]);
        const double zhi = sqrt(zhi2);
        const double zlo2 = dlo2 - rho2;
        const double zlo = zlo2 > 0.0 ? sqrt(zlo2) : 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const double bk = (k ? -sz : sz) - rz;
          int alo = rir_floor((-zhi - bk) / twoLz) - 1, ahi, blo, bhi;
          if (zlo > 0.0) {   // pz in [-zhi, -zlo] and in [zlo, zhi]
            ahi = rir_floor((-zlo - bk) / twoLz) + 1;
            blo = rir_floor((zlo - bk) / twoLz) - 1;
            bhi = rir_floor((zhi - bk) / twoLz) + 1;
          } else {           // pz in [-zhi, zhi]: one run
            ahi = rir_floor((zhi - bk) / twoLz) + 1;
            blo = 1;
            bhi = 0;
          }
          alo = alo > -lim ? alo : -lim;
          ahi = ahi < lim ? ahi : lim;
          bhi = bhi < lim ? bhi : lim;
          blo = blo > ahi ? blo : ahi + 1;   // disjoint: no image twice
          m0[2 * k] = alo;
          cn[2 * k] = ahi >= alo ? ahi - alo + 1 : 0;
          m0[2 * k + 1] = blo;
          cn[2 * k + 1] = bhi >= blo ? bhi - blo + 1 : 0;
        }
      }
    }
    // the candidates numbered in column order: an exclusive prefix sum over the 256 columns
    const int tot = (cn[0] + cn[1]) + (cn[2] + cn[3]);
    int v = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(v, o, 64);
      if (lane >= o) v += u;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) base += wsum[w];
      total += wsum[w];
    }
    c_pre[j] = base + v - tot;
    c_rho2[j] = rho2;
    c_axy[j] = axy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c_m0[j][i] = m0[i];
      c_cn[j][i] = cn[i];
    }
    __syncthreads();
    for (int e0 = 0; e0 < total; e0 += RIR_TILE) {
      const int e = e0 + j;
      bool take = false;
      int n0 = 0;
      double f = 0.0, a = 0.0;
      if (e < total) {
        int lo = 0, hi = RIR_TILE - 1;   // the last column whose first candidate is at or before e
        while (lo < hi) {
          const int mid = (lo + hi + 1) >> 1;
          if (c_pre[mid] <= e)
            lo = mid;
          else
            hi = mid - 1;
        }
        int o = e - c_pre[lo], run = 0;
        while (run < 3 && o >= c_cn[lo][run]) {
          o -= c_cn[lo][run];
          ++run;
        }
        const int m = c_m0[lo][run] + o, k = run >> 1;
        const double pz = ((k ? -sz : sz) - rz) + (double)(2 * m) * Lz;
        const double d = sqrt(c_rho2[lo] + pz * pz);
        const double tau = d * rate;
        const double fl = floor(tau);
        if (fl - (double)Hw + 1.0 <= (double)(tend - 1) && fl + (double)Hw >= (double)t0) {
          take = true;
          n0 = (int)fl;
          f = tau - fl;
          const double az = tb[4 * stride + abs(m - k)] * tb[5 * stride + abs(m)];
          a = (c_axy[lo] * az) / ((4.0 * M_PI) * d);
          const int first = n0 - Hw + 1 > 0 ? n0 - Hw + 1 : 0;
          if (first >= t0) ++cnt;   // first <= tend - 1 holds: this tile counts the image
        }
      }
      const unsigned long long bal = __ballot(take);
      const int pos = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wacc[wave] = __popcll(bal);
      __syncthreads();
      int off = 0, nacc = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w < wave) off += wacc[w];
        nacc += wacc[w];
      }
      if (take) {
        const int i = off + pos;
        double sf, cf;
        sincos((M_PI * f) / (double)Hw, &sf, &cf);
        l_n0[i] = n0;
        l_f[i] = f;
        l_a[i] = a;
        l_sp[i] = sin(M_PI * f);
        l_cf[i] = cf;
        l_sf[i] = sf;
      }
      __syncthreads();
      if (t < len) {
        for (int i = 0; i < nacc; ++i) {
          const int kp = t - l_n0[i];
          if (kp > -Hw && kp <= Hw) {
            const double x = (double)kp - l_f[i];
            if (fabs(x) < (double)Hw) {
              const double2 w = cs[kp + Hw - 1];
              const double win = 0.5 * (1.0 + (w.x * l_cf[i] + w.y * l_sf[i]));
              double sinc = 1.0;
              if (x != 0.0) sinc = ((kp & 1) ? l_sp[i] : -l_sp[i]) / (M_PI * x);
              acc += (l_a[i] * win) * sinc;
            }
          }
        }
      }
    }
  }
  if (t < T) hr[t] = t < len ? acc : 0.0;
  if (tilecount) {   // uniform
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (j == 0) tilecount[(size_t)r * tiles + tile] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
  }
}

__global__ __launch_bounds__(64) void rir_count_kernel(const long long* __restrict__ tilecount,
                                                       int tiles, long long* __restrict__ images) {
  const int r = blockIdx.x;
  long long v = 0;
  for (int i = threadIdx.x; i < tiles; i += 64) v += tilecount[(size_t)r * tiles + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if (threadIdx.x == 0) images[r] = v;
}

inline bool rir_sizes_ok(int count, int T) {
  return count > 0 && count <= 65535 && T > 0 && T <= SEGAN_RIR_MAX_T;
}

inline long long rir_geom_bytes(int count) { return (long long)count * SEGAN_RIR_GEOM * 8; }

}  // namespace

extern "C" int segan_rir_dims(int count, int T, int srate, long long* out) {
  int Hw = 0;
  SEGAN_REQUIRE(out, "rir: NULL pointer");
  SEGAN_REQUIRE(rir_sizes_ok(count, T) && rir_rate(srate, &Hw),
                "rir: bad sizes count=%d T=%d srate=%d", count, T, srate);
  const int tiles = ceil_div(T, RIR_TILE);
  out[0] = Hw;
  out[1] = rir_stride(T, Hw, (double)srate / RIR_C);
  out[2] = tiles;
  out[3] = rir_geom_bytes(count) + (long long)count * tiles * 8;
  return SEGAN_OK;
}

extern "C" int segan_rir(const double* geom, const double* tables, const int* lengths, int count,
                         int T, int srate, double* h, long long* images, void* ws, void* stream) {
  int Hw = 0;
  SEGAN_REQUIRE(geom && tables && h && ws, "rir: NULL pointer");
  SEGAN_REQUIRE(rir_sizes_ok(count, T) && rir_rate(srate, &Hw),
                "rir: bad sizes count=%d T=%d srate=%d", count, T, srate);
  SEGAN_REQUIRE((((uintptr_t)geom | (uintptr_t)tables | (uintptr_t)h | (uintptr_t)images |
                  (uintptr_t)ws) & 7) == 0 && ((uintptr_t)lengths & 3) == 0,
                "rir: a pointer is not aligned to its element");
  for (int i = 0; i < count; ++i) {
    const double* g = geom + (size_t)i * SEGAN_RIR_GEOM;
    double dist2 = 0.0;
    for (int w = 0; w < 3; ++w) {
      const double L = g[w], s = g[3 + w], r = g[6 + w];
      SEGAN_REQUIRE(L >= 1.0 && L <= 50.0, "rir: room %d: side %d of %g m is not in 1 .. 50", i, w,
                    L);
      SEGAN_REQUIRE(s > 0.0 && s < L && r > 0.0 && r < L,
                    "rir: room %d: source and receiver must lie strictly inside the room "
                    "(axis %d: %g and %g of %g m)", i, w, s, r, L);
      dist2 += (s - r) * (s - r);
    }
    SEGAN_REQUIRE(dist2 >= 0.05 * 0.05,
                  "rir: room %d: source and receiver are %g m apart, below 0.05 m", i,
                  sqrt(dist2));
    for (int w = 0; w < 6; ++w)
      SEGAN_REQUIRE(g[9 + w] >= 0.0 && g[9 + w] <= 1.0,
                    "rir: room %d: beta %d of %g is not in 0 .. 1", i, w, g[9 + w]);
  }
  const RirTable* tb = rir_table(srate);
  if (!tb) return SEGAN_ELAUNCH;
  hipStream_t st = (hipStream_t)stream;
  const double rate = (double)srate / RIR_C;
  const int tiles = ceil_div(T, RIR_TILE);
  double* dgeom = (double*)ws;
  long long* tilecount = images ? (long long*)((char*)ws + rir_geom_bytes(count)) : nullptr;
  // in stream order, and read before the call returns: geom is the caller's to free
  if (hipMemcpyWithStream(dgeom, geom, (size_t)rir_geom_bytes(count), hipMemcpyHostToDevice, st) !=
      hipSuccess) {
    segan_set_error("rir: the copy of the geometry failed");
    return SEGAN_ELAUNCH;
  }
  hipLaunchKernelGGL(rir_kernel, dim3(tiles, count), dim3(RIR_TILE), 0, st,
                     (const double*)dgeom, tables, rir_stride(T, Hw, rate), lengths, T, Hw, rate,
                     (const double2*)tb->cs, h, tilecount);
  if (int e = segan_check_launch("rir_kernel")) return e;
  if (images) {
    hipLaunchKernelGGL(rir_count_kernel, dim3(count), dim3(64), 0, st,
                       (const long long*)tilecount, tiles, images);
    return segan_check_launch("rir_count_kernel");
  }
  return SEGAN_OK;
}
