/*
 * segan_dereverb.h — extension header of libsegan_hip.so: the WPE dereverberation baseline
 * (DESIGN.md section 21).
 *
 * The exports below are purely additive: SEGAN_ABI_VERSION stays 17 and include/segan_hip.h is
 * unchanged.  They live in a header of their own because the main header's set of declarations
 * and macros is pinned by the tests of ABI 17 (the count of its entry points among them): a
 * caller of ABI 17 sees exactly the header it was built against, and a caller that wants WPE
 * includes this file as well.  The conventions are the main header's (device pointers owned by
 * the caller, `stream` a hipStream_t as void*, 0 on success, negative on error with the message in
 * segan_last_error(), here prefixed `wpe:`); the binding reads this file with the same reader
 * (segan_pytorch_amd/_lib.py: EXT_SIGNATURES, EXT_DEFINES).
 *
 * WPE, weighted prediction error (Nakatani et al., IEEE TASLP 2010), single channel, in the STFT
 * domain, defined by scripts/wpe_oracle.py.  Rows x [rows][T] of x_dtype (SEGAN_DT_F32 or
 * SEGAN_DT_F64) at srate 16000 or 8000, row r restricted to its first lengths[r] samples L (device
 * int[rows], clamped to 0 .. T; NULL: all T); all arithmetic fp64.  K = taps, D = delay.
 *   N = 512, H = 128 at 16 kHz (256, 64 at 8 kHz), F = N / 2 + 1; w[n] = sqrt(0.5 - 0.5 cos(2 pi n
 *     / N)) for analysis and synthesis; nf = ceil(L / H) + 3 frames, frame j over the samples
 *     (j - 3) H .. (j - 3) H + N - 1, zero outside [0, L); Y[k][j] = the DFT of the windowed frame.
 *   nf <= D + K or L = 0: y = x below L (a copy), X = Y, g = 0.
 *   Per bin k, X = Y and g = 0 at the start, `iterations` times: p_t = |X_t|^2, m = max_t p_t
 *     (m = 0: g = 0, the bin stops); lambda_t = max(p_t, 1e-10 m); y~_t = (Y_{t-D} .. Y_{t-D-K+1}),
 *     zeros before the first frame; R = sum_t y~_t y~_t^H / lambda_t, P = sum_t y~_t conj(Y_t) /
 *     lambda_t, every sum in ascending t (tr R = 0: g = 0, the bin stops); R += 1e-10 (tr R / K) I;
 *     g = R^-1 P by an unpivoted lower Cholesky (a pivot that is not positive: g = 0, the bin
 *     stops, SEGAN_WPE_ST_PIVOT is set in status[r]); X_t = Y_t - g^H y~_t.
 *   y = the inverse real DFT of each X[:, j] (imaginary parts of the bins 0 and N / 2 ignored)
 *     times w, the four frames over a sample added with the earlier frame first, times 1 / 2; zero
 *     from L to T.
 *   segan_wpe_dims (host only): out[5] = {N, H, F, nf of a row of T samples, the bytes of
 *     workspace `ws` for `rows` rows: 32 F nf for Y and X, and 4 F rounded up to 16 for the bins'
 *     flags, a row}.
 *   segan_wpe: y [rows][T] of y_dtype (SEGAN_DT_F64, or SEGAN_DT_F32 rounded once), nframes
 *     int[rows] (each row's own nf), status int[rows] (0 or SEGAN_WPE_ST_PIVOT).  Optional (NULL)
 *     stage outputs, complex fp64 as (re, im) pairs: Y_out and X_out [rows][F][nf of T] (the STFT
 *     and the filtered STFT, bin-major, zero from the row's own nf on), g_out [rows][F][taps] (the
 *     last filter).  ws: 16-byte aligned.
 * No atomics, no scratch, every sum in an order fixed by the indices: a row's bits depend neither
 * on T, nor on the other rows, nor on the samples past its length, nor on the frame tile the hot
 * kernel streams long rows with (SEGAN_WPE_TILE frames).  rows in 1 .. 65535, T in 1 .. 2^24, taps
 * in 1 .. SEGAN_WPE_MAX_TAPS, delay in 1 .. SEGAN_WPE_MAX_DELAY, iterations in 0 ..
 * SEGAN_WPE_MAX_ITERATIONS, checked before any launch.
 */
#ifndef SEGAN_DEREVERB_H
#define SEGAN_DEREVERB_H

#ifdef __cplusplus
extern "C" {
#endif

#define SEGAN_WPE_MAX_TAPS 32
#define SEGAN_WPE_MAX_DELAY 8
#define SEGAN_WPE_MAX_ITERATIONS 8
#define SEGAN_WPE_TILE 512
#define SEGAN_WPE_ST_PIVOT 2
int segan_wpe_dims(int rows, int T, int srate, int taps, int delay, long long* out);
int segan_wpe(const void* x, int x_dtype, const int* lengths, int rows, int T, int srate, int taps,
              int delay, int iterations, void* y, int y_dtype, int* nframes, int* status,
              double* Y_out, double* X_out, double* g_out, void* ws, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGAN_DEREVERB_H */
