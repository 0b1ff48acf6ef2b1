/*
 * segan_pyin.h — extension header of libsegan_hip.so: the Viterbi-smoothed pitch tracker
 * (pYIN-style).
 *
 * The exports below are purely additive: SEGAN_ABI_VERSION stays 17, and include/segan_hip.h and
 * include/segan_dereverb.h are unchanged.  The conventions are the main header's (device pointers
 * owned by the caller, `stream` a hipStream_t as void*, 0 on success, negative on error with the
 * message in segan_last_error(), here prefixed `pyin:`); the binding reads this file with the same
 * reader (segan_pytorch_amd/_lib.py: PYIN_SIGNATURES, PYIN_DEFINES).
 *
 * pYIN (Mauch & Dixon, ICASSP 2014) on segan_pitch's framing (hop, frame, tau_min, tau_max, rates
 * and frame count are segan_pitch's), defined by scripts/pyin_oracle.py.  All arithmetic is fp64
 * and no transcendental function runs on the device: the tables are built on the host, and the
 * decoder works on scaled probabilities.  M = SEGAN_PYIN_BINS, W = SEGAN_PYIN_W.
 *   Tables (segan_pyin_tables writes them to host memory; the kernels read the same bits):
 *     C[0 .. SEGAN_PYIN_NTHETA]: C[0] = 0, C[i] the ascending running sum of w_k / sum(w), w_k =
 *       theta_k (1 - theta_k)^17, theta_k = k / 100: the Beta(2, 18) prior of the thresholds.
 *     edge[0 .. M]: the bin edges as periods in samples, srate / (60 2^(m / 60)), descending (5 bins
 *       per semitone from 60 Hz).  A period p falls into bin (number of edges >= p) - 1, clamped.
 *     A[2][2 W + 1]: A[s][k + W] = (s ? 0.01 : 0.99) (W + 1 - |k|) / (W + 1)^2, truncated at the
 *       ends of the bin range, not renormalised.
 *   Candidates of a frame with c(tau_max + 1) > 0: YIN's pick under each threshold theta_i; the
 *     thresholds that pick the lag tau form one index range (lo, hi] with the mass C[hi] - C[lo];
 *     the thresholds 1 .. n0 that find no lag give 0.01 C[n0] to the lowest lag of minimal d', added
 *     after that lag's range mass.  Period p = tau + delta by segan_pitch's parabola.  V = the sum
 *     of the masses in ascending lag order, U = max(1 - V, 2^-40).
 *   Observation: B_v(m) = the masses of the candidates of bin m in ascending lag order, B_u(m) =
 *     U / M.
 *   Decoder: state j = v M + m (v = 0 voiced, 1 unvoiced); delta_0 = B_0; for t >= 1 the
 *     predecessors i in ascending state index over the two bands |m_i - m_j| <= W; a strictly
 *     larger delta_{t-1}(i) A[v_i != v_j][m_j - m_i + W] replaces the best; delta_t(j) = best
 *     B_t(j); after each frame delta_t times 2^-e, e the binary exponent of its maximum.  The
 *     lowest index of maximal delta_{F-1} ends the path; then the backtrace.
 *   Output under segan_pitch's contract (segan_f0_eval consumes f0 and lag unchanged): a decoded
 *     voiced state (0, m) yields the frame's candidate of bin m with the largest mass (lowest lag
 *     on ties), f0 = srate / p, lag = tau; otherwise f0 = 0, lag = 0; vprob = V (0 for a frame
 *     without candidates).  Frames from the row's own count on: f0 = 0, lag = -1, vprob = NaN.
 *   segan_pyin_tables (host only): C [101], edge [M + 1], A [2][2 W + 1] of host memory.
 *   segan_pyin_dims (host only): out[2] = {frames F of a row of T samples, the doubles of workspace
 *     `ws` for `rows` rows}.
 *   segan_pyin: x [rows][T] fp32, lengths int[rows] (device; NULL: all T), f0 / vprob fp64
 *     [rows][F], lag int [rows][F].  Optional (NULL) stage outputs: bv_out fp64 [rows][F][M] (NaN
 *     from the row's own frame count on), state_out int [rows][F] (the decoded state, -1 from the
 *     row's count on), delta_out fp64 [rows][2 M] (the last frame's scaled delta, NaN for a row
 *     without a frame).  ws: 8-byte aligned.
 * No atomics, no scratch, every sum in an order fixed by the indices: a row's bits depend neither
 * on T, nor on the other rows, nor on the samples past its length, and a row times a power of two
 * gives the same bits.  rows in 1 .. 65535, T in 1 .. 2^24, srate 16000 or 8000, checked before
 * any launch.
 */
#ifndef SEGAN_PYIN_H
#define SEGAN_PYIN_H

#ifdef __cplusplus
extern "C" {
#endif

#define SEGAN_PYIN_NTHETA 100
#define SEGAN_PYIN_BINS 165
#define SEGAN_PYIN_W 11
int segan_pyin_tables(int srate, double* C, double* edge, double* A);
int segan_pyin_dims(int rows, int T, int srate, long long* out);
int segan_pyin(const float* x, const int* lengths, int rows, int T, int srate, double* f0, int* lag,
               double* vprob, double* bv_out, int* state_out, double* delta_out, double* ws,
               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGAN_PYIN_H */
