// Viterbi-smoothed pitch tracking (pYIN, Mauch & Dixon 2014) on segan_pitch's framing (DESIGN.md
// section 22, include/segan_pyin.h, scripts/pyin_oracle.py).  fp64, no transcendental function on
// the device (the tables are the host's), no atomics, every sum and every comparison in an order
// fixed by the indices alone: device and oracle perform the same IEEE operations.
//
//   pitch kernels           segan_pitch.hip's, through segan_pitch_cmnd_ctot: d' of every frame
//                           and lag, and c(tau_max + 1) of every frame, into the workspace
//   pyin_candidate_kernel   one wave per (frame, row): the descent stops, the prefix minimum that
//                           gives each stop its range of thresholds, the masses, the parabola, the
//                           bin search; writes B_v [F][M], V [F] and each bin's best candidate
//   pyin_viterbi_kernel     one workgroup per row, one state per lane: the forward recursion with
//                           one barrier per frame (delta double-buffered in LDS, the power-of-two
//                           scale of frame t - 1 applied when it is read), a one-byte psi per
//                           state and frame in the workspace, then the backtrace by one thread and
//                           the output stage by all
#include "segan_signal.h"
#include "../../include/segan_pyin.h"

// nothing below may be contracted: the oracle rounds every product and every sum on its own
#pragma clang fp contract(off)

#define PYIN_NT SEGAN_PYIN_NTHETA
#define PYIN_M SEGAN_PYIN_BINS
#define PYIN_W SEGAN_PYIN_W
#define PYIN_S (2 * PYIN_M)            // states: voiced bins, then unvoiced bins
#define PYIN_SPAN (2 * PYIN_W + 1)     // predecessors per band
#define PYIN_CAND_WAVES 4              // frames per workgroup of pyin_candidate_kernel
#define PYIN_VIT_THREADS 384
#define PYIN_VIT_WAVES (PYIN_VIT_THREADS / 64)
#define PYIN_PER_LANE 4                // lags per lane of the candidate kernel: 256 >= 227
// the device table: C, then edge, then A
#define PYIN_TAB_EDGE (PYIN_NT + 1)
#define PYIN_TAB_A (PYIN_TAB_EDGE + PYIN_M + 1)
#define PYIN_TAB_SIZE (PYIN_TAB_A + 2 * PYIN_SPAN)
#define PYIN_P_A 0.01
#define PYIN_FLOOR 0x1p-40

static_assert(PYIN_S <= PYIN_VIT_THREADS, "one state per lane");
static_assert(64 * PYIN_PER_LANE >= 266 - 40 + 1, "every lag of tau_min .. tau_max has a lane");
static_assert(2 * PYIN_SPAN <= 255, "psi is one byte");

namespace {

// the workspace of `rows` rows, offsets in doubles
struct PyinLayout {
  size_t pitch, cmnd, ctot, bv, V, bestp, besttau, state, psi, total;
};

PyinLayout pyin_layout(int rows, int T, const PitchRate& pr) {
  const size_t nb = pitch_blocks(T, pr.H, pr.nl), F = pitch_frames_of((int)nb), R = rows;
  PyinLayout l;
  size_t o = 0;
  l.pitch = o, o += R * nb * 2 * pr.nl;
  l.cmnd = o, o += R * F * pr.nl;
  l.ctot = o, o += R * F;
  l.bv = o, o += R * F * PYIN_M;
  l.V = o, o += R * F;
  l.bestp = o, o += R * F * PYIN_M;
  l.besttau = o, o += (R * F * PYIN_M + 1) / 2;
  l.state = o, o += (R * F + 1) / 2;
  l.psi = o, o += (R * F * PYIN_S + 7) / 8;
  l.total = o;
  return l;
}

// how many of the thresholds i / 100, i = 1 .. 100, are <= v (that is, do not have v < theta_i)
__device__ __forceinline__ int pyin_at_most(double v) {
  int k = v > 0.0 ? (v < 1.0 ? (int)(v * 100.0) : PYIN_NT) : 0;   // within one of the answer
  if (k < PYIN_NT && (double)(k + 1) / 100.0 <= v) ++k;
  if (k > 0 && (double)k / 100.0 > v) --k;
  return k;
}

// min over the lanes below this one (+inf for lane 0)
__device__ __forceinline__ double pyin_excl_min(double x, int lane) {
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_up(x, o, 64);
    if (lane >= o) x = y < x ? y : x;
  }
  const double y = __shfl_up(x, 1, 64);
  return lane ? y : __builtin_inf();
}

// Frame PYIN_CAND_WAVES blockIdx.x + wave of row blockIdx.y.  bv / bestp / besttau [rows][F][M]
// and V [rows][F] are written for the row's own frames; bv_out (optional) for all F, NaN past them.
__global__ __launch_bounds__(64 * PYIN_CAND_WAVES) void pyin_candidate_kernel(
    const int* __restrict__ lengths, int T, PitchRate pr, int F, const double* __restrict__ tab,
    const double* __restrict__ cmnd, const double* __restrict__ ctot, double* __restrict__ bv,
    double* __restrict__ V, double* __restrict__ bestp, int* __restrict__ besttau,
    double* __restrict__ bv_out) {
  __shared__ double tabs[PYIN_TAB_A];   // C, edge
  __shared__ double dd[PYIN_CAND_WAVES][PITCH_MAX_LAGS];
  __shared__ double sbv[PYIN_CAND_WAVES][PYIN_M], sbm[PYIN_CAND_WAVES][PYIN_M];
  __shared__ double sbp[PYIN_CAND_WAVES][PYIN_M];
  __shared__ int sbt[PYIN_CAND_WAVES][PYIN_M];
  const int r = blockIdx.y, w = threadIdx.x >> 6, lane = threadIdx.x & 63, nl = pr.nl;
  const int L = segan_row_samples(lengths, r, T);
  int nf = pitch_frames_of(pitch_blocks(L, pr.H, nl));
  if (nf > F) nf = F;
  const int t = blockIdx.x * PYIN_CAND_WAVES + w;
  const bool in = t < F, active = t < nf;
  const size_t fr = (size_t)r * F + (in ? t : 0);
  for (int i = threadIdx.x; i < PYIN_TAB_A; i += 64 * PYIN_CAND_WAVES) tabs[i] = tab[i];
  double* d = dd[w];
  for (int i = lane; i < nl; i += 64) d[i] = active ? cmnd[fr * nl + i] : 1.0;
  for (int i = lane; i < PYIN_M; i += 64) {
    sbv[w][i] = 0.0;
    sbm[w][i] = 0.0;
    sbp[w][i] = 0.0;
    sbt[w][i] = 0;
  }
  const bool has = active && ctot[fr] > 0.0;
  __syncthreads();
  const double* C = tabs;
  const double* edge = tabs + PYIN_TAB_EDGE;
  const double inf = __builtin_inf();

  // the prefix minimum pm(k) of d' over tau_min .. k
  const int k0 = pr.tmin + PYIN_PER_LANE * lane;
  double v[PYIN_PER_LANE], pm[PYIN_PER_LANE], prev[PYIN_PER_LANE], mass[PYIN_PER_LANE];
  bool stop[PYIN_PER_LANE];
  double run = inf;
#pragma unroll
  for (int j = 0; j < PYIN_PER_LANE; ++j) {
    const int k = k0 + j;
    v[j] = k <= pr.tmax ? d[k] : inf;
    run = v[j] < run ? v[j] : run;
    pm[j] = run;
  }
  double ex = pyin_excl_min(run, lane);
#pragma unroll
  for (int j = 0; j < PYIN_PER_LANE; ++j) pm[j] = ex < pm[j] ? ex : pm[j];
  const double gmin = __shfl(pm[PYIN_PER_LANE - 1], 63, 64);
  // a descent stops at k = tau_max or where d'(k + 1) < d'(k) fails; the thresholds that stop at
  // k are those above pm(k) and at most pm(the stop before k): prev(k), +inf for the first stop
  run = inf;
#pragma unroll
  for (int j = 0; j < PYIN_PER_LANE; ++j) {
    const int k = k0 + j;
    stop[j] = k <= pr.tmax && (k == pr.tmax || !(d[k + 1] < d[k]));
    prev[j] = run;
    const double s = stop[j] ? pm[j] : inf;
    run = s < run ? s : run;
  }
  ex = pyin_excl_min(run, lane);
#pragma unroll
  for (int j = 0; j < PYIN_PER_LANE; ++j) prev[j] = ex < prev[j] ? ex : prev[j];
  // the lowest lag of minimal d' (a stop: nothing below it follows) takes the thresholds without
  // a lag
  int myj = -1;
#pragma unroll
  for (int j = PYIN_PER_LANE - 1; j >= 0; --j)
    if (k0 + j <= pr.tmax && v[j] == gmin) myj = j;
  const unsigned long long holders = __ballot(myj >= 0);
  const int star_lane = holders ? __ffsll((long long)holders) - 1 : 0;
  const int star_j = __shfl(myj, star_lane, 64);
  const int n0 = pyin_at_most(gmin);
  bool any = false;
  double per[PYIN_PER_LANE];
  int bin[PYIN_PER_LANE];
#pragma unroll
  for (int j = 0; j < PYIN_PER_LANE; ++j) {
    double m = 0.0;
    if (has && stop[j]) {
      m = C[pyin_at_most(prev[j])] - C[pyin_at_most(pm[j])];
      if (n0 > 0 && lane == star_lane && j == star_j) m = m + PYIN_P_A * C[n0];
    }
    mass[j] = m;
    per[j] = 0.0;
    bin[j] = 0;
    if (m > 0.0) {
      any = true;
      const int k = k0 + j;
      const double ya = d[k - 1], yb = d[k], yc = d[k + 1];
      const double den = ya - 2.0 * yb + yc;
      double delta = 0.0;
      if (den > 0.0) {
        delta = 0.5 * (ya - yc) / den;
        delta = delta < -0.5 ? -0.5 : (delta > 0.5 ? 0.5 : delta);
      }
      const double p = (double)k + delta;
      int lo = 0, hi = PYIN_M + 1;   // the number of edges >= p (they descend)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (edge[mid] >= p) lo = mid + 1;
        else hi = mid;
      }
      const int b = lo - 1;
      per[j] = p;
      bin[j] = b < 0 ? 0 : (b > PYIN_M - 1 ? PYIN_M - 1 : b);
    }
  }
  // the candidates in ascending lag order: V, each bin's sum and its candidate of largest mass
  double Vsum = 0.0;
  unsigned long long todo = __ballot(any);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
#pragma unroll
    for (int j = 0; j < PYIN_PER_LANE; ++j) {
      const double m = __shfl(mass[j], src, 64);
      const double p = __shfl(per[j], src, 64);
      const int b = __shfl(bin[j], src, 64);
      if (m > 0.0) {
        Vsum = Vsum + m;
        if (lane == 0) {
          sbv[w][b] = sbv[w][b] + m;
          if (m > sbm[w][b]) {
            sbm[w][b] = m;
            sbp[w][b] = p;
            sbt[w][b] = pr.tmin + PYIN_PER_LANE * src + j;
          }
        }
      }
    }
  }
  __syncthreads();
  if (active) {
    for (int i = lane; i < PYIN_M; i += 64) {
      bv[fr * PYIN_M + i] = sbv[w][i];
      bestp[fr * PYIN_M + i] = sbp[w][i];
      besttau[fr * PYIN_M + i] = sbt[w][i];
      if (bv_out) bv_out[fr * PYIN_M + i] = sbv[w][i];
    }
    if (lane == 0) V[fr] = Vsum;
  } else if (in && bv_out) {
    for (int i = lane; i < PYIN_M; i += 64) bv_out[fr * PYIN_M + i] = NAN;
  }
}

__device__ __forceinline__ double pyin_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(v, o, 64);
    v = y > v ? y : v;
  }
  return v;
}

// 2^-e with e the binary exponent of the largest of the waves' maxima
__device__ __forceinline__ double pyin_scale(const double* wm) {
  double mx = wm[0];
#pragma unroll
  for (int i = 1; i < PYIN_VIT_WAVES; ++i) mx = wm[i] > mx ? wm[i] : mx;
  int e;
  frexp(mx, &e);
  return ldexp(1.0, -e);
}

// Row blockIdx.x.  psi [rows][F][2 M] bytes (band offset + SPAN * switched) and state [rows][F]
// are workspace; f0 / lag / vprob [rows][F] are written for all F frames.
__global__ __launch_bounds__(PYIN_VIT_THREADS) void pyin_viterbi_kernel(
    const int* __restrict__ lengths, int T, int srate, PitchRate pr, int F,
    const double* __restrict__ tab, const double* __restrict__ bv, const double* __restrict__ V,
    const double* __restrict__ bestp, const int* __restrict__ besttau, unsigned char* psi,
    int* state, double* __restrict__ f0, int* __restrict__ lag, double* __restrict__ vprob,
    int* __restrict__ state_out, double* __restrict__ delta_out) {
  __shared__ double dl[2][PYIN_VIT_THREADS];
  __shared__ double wm[2][PYIN_VIT_WAVES];
  const int r = blockIdx.x, j = threadIdx.x, wave = j >> 6, lane = j & 63;
  const bool act = j < PYIN_S;
  const int vj = act && j >= PYIN_M ? 1 : 0, mj = act ? j - vj * PYIN_M : 0;
  const int L = segan_row_samples(lengths, r, T);
  int nf = pitch_frames_of(pitch_blocks(L, pr.H, pr.nl));
  if (nf > F) nf = F;
  const size_t row = (size_t)r * F;
  const double* bvr = bv + row * PYIN_M;
  const double* Vr = V + row;
  unsigned char* psir = psi + row * PYIN_S;
  int* str = state + row;

  // A[v_i != v_j] of the voiced and of the unvoiced predecessors, by band position
  double Av[PYIN_SPAN], Au[PYIN_SPAN];
#pragma unroll
  for (int k = 0; k < PYIN_SPAN; ++k) {
    Av[k] = tab[PYIN_TAB_A + vj * PYIN_SPAN + k];
    Au[k] = tab[PYIN_TAB_A + (1 - vj) * PYIN_SPAN + k];
  }
  // B_t(j): the bin's mass, or U / M
  auto obs = [&](int t) -> double {
    if (!act) return 0.0;
    if (!vj) return bvr[(size_t)t * PYIN_M + mj];
    const double u = 1.0 - Vr[t];
    return (u > PYIN_FLOOR ? u : PYIN_FLOOR) / (double)PYIN_M;
  };

  if (nf > 0) {   // uniform over the workgroup
    double b = obs(0);
    dl[0][j] = b;
    b = pyin_wave_max(b);
    if (lane == 0) wm[0][wave] = b;
    double bnext = nf > 1 ? obs(1) : 0.0;
    __syncthreads();
    for (int t = 1; t < nf; ++t) {
      const double* pv = dl[(t - 1) & 1];
      const double s = pyin_scale(wm[(t - 1) & 1]);
      b = bnext;
      if (t + 1 < nf) bnext = obs(t + 1);
      double best = -1.0;
      int code = 0;
#pragma unroll
      for (int k = 0; k < PYIN_SPAN; ++k) {      // voiced predecessors, ascending bin
        const int mi = mj + k - PYIN_W;
        const bool ok = mi >= 0 && mi < PYIN_M;
        const double val = (pv[ok ? mi : 0] * s) * Av[PYIN_SPAN - 1 - k];
        if (ok && val > best) {
          best = val;
          code = k + vj * PYIN_SPAN;
        }
      }
#pragma unroll
      for (int k = 0; k < PYIN_SPAN; ++k) {      // unvoiced predecessors
        const int mi = mj + k - PYIN_W;
        const bool ok = mi >= 0 && mi < PYIN_M;
        const double val = (pv[PYIN_M + (ok ? mi : 0)] * s) * Au[PYIN_SPAN - 1 - k];
        if (ok && val > best) {
          best = val;
          code = k + (1 - vj) * PYIN_SPAN;
        }
      }
      const double dn = act ? best * b : 0.0;
      dl[t & 1][j] = dn;
      if (act) psir[(size_t)t * PYIN_S + j] = (unsigned char)code;
      const double m = pyin_wave_max(dn);
      if (lane == 0) wm[t & 1][wave] = m;
      __syncthreads();
    }
    const int last = (nf - 1) & 1;
    const double s = pyin_scale(wm[last]);
    if (act && delta_out) delta_out[(size_t)r * PYIN_S + j] = dl[last][j] * s;
    if (j == 0) {
      int st = 0;
      double top = dl[last][0];
      for (int i = 1; i < PYIN_S; ++i)
        if (dl[last][i] > top) {
          top = dl[last][i];
          st = i;
        }
      for (int t = nf - 1; t >= 1; --t) {
        str[t] = st;
        const int code = psir[(size_t)t * PYIN_S + st];
        const int sw = code >= PYIN_SPAN ? 1 : 0, off = code - sw * PYIN_SPAN;
        const int v = st >= PYIN_M ? 1 : 0, m = st - v * PYIN_M;
        st = (v ^ sw) * PYIN_M + (m + off - PYIN_W);
      }
      str[0] = st;
    }
    __syncthreads();
  } else if (act && delta_out) {
    delta_out[(size_t)r * PYIN_S + j] = NAN;
  }
  for (int t = j; t < F; t += PYIN_VIT_THREADS) {
    const size_t o = row + t;
    double f = 0.0, vp = NAN;
    int tau = -1, st = -1;
    if (t < nf) {
      st = str[t];
      tau = 0;
      vp = Vr[t];
      if (st < PYIN_M) {
        f = (double)srate / bestp[o * PYIN_M + st];
        tau = besttau[o * PYIN_M + st];
      }
    }
    f0[o] = f;
    lag[o] = tau;
    vprob[o] = vp;
    if (state_out) state_out[o] = st;
  }
}

void pyin_host_tables(int srate, double* C, double* edge, double* A) {
  double w[PYIN_NT + 1], tot = 0.0;
  for (int k = 0; k <= PYIN_NT; ++k) {
    const double th = (double)k / (double)PYIN_NT, q = 1.0 - th;
    const double q2 = q * q, q4 = q2 * q2, q8 = q4 * q4, q16 = q8 * q8;
    w[k] = th * (q16 * q);
  }
  for (int k = 1; k <= PYIN_NT; ++k) tot += w[k];
  C[0] = 0.0;
  for (int k = 1; k <= PYIN_NT; ++k) C[k] = C[k - 1] + w[k] / tot;
  for (int m = 0; m <= PYIN_M; ++m) edge[m] = (double)srate / (60.0 * exp2((double)m / 60.0));
  for (int s = 0; s < 2; ++s)
    for (int k = -PYIN_W; k <= PYIN_W; ++k)
      A[s * PYIN_SPAN + k + PYIN_W] = (s ? 0.01 : 0.99) * (double)(PYIN_W + 1 - (k < 0 ? -k : k)) /
                                      (double)((PYIN_W + 1) * (PYIN_W + 1));
}

struct PyinTables {
  int device, srate;
  double* tab;
};

SeganDeviceTables<PyinTables> g_pyin_tables;

const PyinTables* pyin_tables(int srate) {
  return g_pyin_tables.get(
      "pyin", [&](const PyinTables& e) { return e.srate == srate; },
      [&](PyinTables* e) {
        std::vector<double> t(PYIN_TAB_SIZE);
        pyin_host_tables(srate, t.data(), t.data() + PYIN_TAB_EDGE, t.data() + PYIN_TAB_A);
        e->srate = srate;
        return segan_upload(&e->tab, t, "pyin");
      });
}

}  // namespace

extern "C" int segan_pyin_tables(int srate, double* C, double* edge, double* A) {
  PitchRate pr;
  SEGAN_REQUIRE(C && edge && A, "pyin: NULL pointer");
  SEGAN_REQUIRE(pitch_rate(srate, &pr), "pyin: bad sizes srate=%d", srate);
  pyin_host_tables(srate, C, edge, A);
  return SEGAN_OK;
}

extern "C" int segan_pyin_dims(int rows, int T, int srate, long long* out) {
  PitchRate pr;
  SEGAN_REQUIRE(out, "pyin: NULL pointer");
  SEGAN_REQUIRE(segan_pitch_sizes_ok(rows, T) && pitch_rate(srate, &pr),
                "pyin: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  out[0] = pitch_frames_of(pitch_blocks(T, pr.H, pr.nl));
  out[1] = (long long)pyin_layout(rows, T, pr).total;
  return SEGAN_OK;
}

extern "C" int segan_pyin(const float* x, const int* lengths, int rows, int T, int srate,
                          double* f0, int* lag, double* vprob, double* bv_out, int* state_out,
                          double* delta_out, double* ws, void* stream) {
  PitchRate pr;
  SEGAN_REQUIRE(x && f0 && lag && vprob && ws, "pyin: NULL pointer");
  SEGAN_REQUIRE(segan_pitch_sizes_ok(rows, T) && pitch_rate(srate, &pr),
                "pyin: bad sizes rows=%d T=%d srate=%d", rows, T, srate);
  hipStream_t st = (hipStream_t)stream;
  const int F = pitch_frames_of(pitch_blocks(T, pr.H, pr.nl));
  if (F == 0) {   // no row has a frame: only the rows' last deltas are there to write
    if (delta_out) {
      const PyinTables* tb = pyin_tables(srate);
      if (!tb) return SEGAN_ELAUNCH;
      hipLaunchKernelGGL(pyin_viterbi_kernel, dim3(rows), dim3(PYIN_VIT_THREADS), 0, st, lengths, T,
                         srate, pr, 0, (const double*)tb->tab, (const double*)ws,
                         (const double*)ws, (const double*)ws, (const int*)ws,
                         (unsigned char*)ws, (int*)ws, f0, lag, vprob, state_out, delta_out);
      return segan_check_launch("pyin_viterbi_kernel");
    }
    return SEGAN_OK;
  }
  const PyinTables* tb = pyin_tables(srate);
  if (!tb) return SEGAN_ELAUNCH;
  const PyinLayout l = pyin_layout(rows, T, pr);
  if (int e = segan_pitch_cmnd_ctot(x, lengths, rows, T, srate, ws + l.cmnd, ws + l.ctot,
                                    ws + l.pitch, st))
    return e;
  hipLaunchKernelGGL(pyin_candidate_kernel, dim3(ceil_div(F, PYIN_CAND_WAVES), rows),
                     dim3(64 * PYIN_CAND_WAVES), 0, st, lengths, T, pr, F, (const double*)tb->tab,
                     (const double*)(ws + l.cmnd), (const double*)(ws + l.ctot), ws + l.bv,
                     ws + l.V, ws + l.bestp, (int*)(ws + l.besttau), bv_out);
  if (int e = segan_check_launch("pyin_candidate_kernel")) return e;
  hipLaunchKernelGGL(pyin_viterbi_kernel, dim3(rows), dim3(PYIN_VIT_THREADS), 0, st, lengths, T,
                     srate, pr, F, (const double*)tb->tab, (const double*)(ws + l.bv),
                     (const double*)(ws + l.V), (const double*)(ws + l.bestp),
                     (const int*)(ws + l.besttau), (unsigned char*)(ws + l.psi),
                     (int*)(ws + l.state), f0, lag, vprob, state_out, delta_out);
  return segan_check_launch("pyin_viterbi_kernel");
}
