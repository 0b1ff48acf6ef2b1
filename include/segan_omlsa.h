/*
 * segan_omlsa.h — extension header of libsegan_hip.so: the OM-LSA enhancer with IMCRA noise
 * tracking.
 *
 * The exports below are purely additive: SEGAN_ABI_VERSION stays 17, and include/segan_hip.h,
 * include/segan_dereverb.h and include/segan_pyin.h are unchanged.  The conventions are the main
 * header's (device pointers owned by the caller, `stream` a hipStream_t as void*, 0 on success,
 * negative on error with the message in segan_last_error(), here prefixed `omlsa:`; x_dtype and
 * y_dtype are SEGAN_DT_F32 or SEGAN_DT_F64 of the main header); the binding reads this file with
 * the same reader (segan_pytorch_amd/_lib.py: OMLSA_SIGNATURES, OMLSA_DEFINES).
 *
 * The optimally-modified log-spectral-amplitude estimator (Cohen & Berdugo 2001) on the noise
 * spectrum of the improved minima-controlled recursive averaging (Cohen 2003), defined by
 * scripts/omlsa_oracle.py.  All arithmetic is fp64, every product and sum rounded on its own.
 *   Framing, window, analysis and synthesis are segan_denoise's: F = srate / 50, H = F / 2,
 *     N = 2 F, the Hamming window scaled by H / sum w, nf = L / H - 1 frames for L >= 6 F and none
 *     below (the row is then copied), spectrum S_t[k], k = 0 .. F, s2 = re^2 + im^2; the output is
 *     the overlap-add of the first F samples of the inverse DFT of G S_t, the earlier frame first,
 *     zero from (nf + 1) H on.
 *   sm3(a)[k] = (0.25 a[k - 1] + 0.5 a[k]) + 0.25 a[k + 1], a[-1] := a[1], a[F + 1] := a[F - 1].
 *   Per frame t and bin k, with as = 0.9, ad = 0.85, a = 0.92, beta = 1.47, Bmin = 1.66, g0 = 4.6,
 *   g1 = 3, z0 = 1.67, U = SEGAN_OMLSA_U, V = SEGAN_OMLSA_V, ln Gmin = ln 10^(-25/20):
 *     1. Sf = sm3(s2); S = Sf (t = 0) or as S + (1 - as) Sf; t = 0: Smin = Smact = S and the U
 *        history slots = S; else Smin = min(Smin, S), Smact = min(Smact, S).
 *     2. th = Bmin Smin; I = (s2 < g0 th) and (S < z0 th).
 *     3. den = sm3(I), num = sm3(I s2); Stf = num / den where den > 0, else the previous St (Sf at
 *        t = 0); St = Stf (t = 0) or as St + (1 - as) Stf; Stmin, Stmact and a second history as
 *        in step 1.
 *     4. tth = Bmin Stmin; low = St < z0 tth; q = 1 where low and s2 <= tth; q = (g1 - s2 / tth) /
 *        (g1 - 1) where low and s2 < g1 tth; q = 0 otherwise.
 *     5. lam = max(beta lbar, 2^-100), lbar = s2 of frame 0 at t = 0; gamma = min(s2 / lam, 40);
 *        xi = max((a P) / lam + (1 - a) max(gamma - 1, 0), 10^-2.5), the first term a at t = 0;
 *        A = xi / (1 + xi); nu = A gamma.
 *     6. p = 0 where q = 1, 1 where q = 0, else 1 / (1 + ((q / (1 - q)) (1 + xi)) exp(-nu)).
 *     7. at = ad + (1 - ad) p; lbar <- at lbar + (1 - at) s2.
 *     8. GH1 = A exp(E1(max(nu, 2^-40)) / 2); G = exp(p ln GH1 + (1 - p) ln Gmin);
 *        P <- (GH1 GH1) s2.
 *     9. If (t + 1) % V == 0: slot j = ((t + 1) / V - 1) % U; history[j] <- Smact; Smin <- the
 *        minimum over the U slots; Smact <- S; the same for the second history.
 *    10. presence_t = ((sum_k c_k p[k]) / F) / 2 with c_0 = c_F = 1, the others 2, the sum in
 *        segan_denoise's order (groups of 64 bins in ascending k, then the groups in ascending
 *        order); rough_t = the number of bins with I = 1.
 *   segan_omlsa_dims (host only): out[5] = {F, H, N, the frames nf of a row of T samples, the
 *     bytes of workspace `ws` for `rows` rows}.
 *   segan_omlsa: x [rows][T] of x_dtype, lengths int[rows] (device; NULL: all T), y [rows][T] of
 *     y_dtype (rounded once), nframes int[rows].  Optional (NULL) outputs: presence fp64
 *     [rows][nf of T] (NaN from the row's own frame count on), rough int [rows][nf of T] (-1 from
 *     the row's own count on), noise fp64 [rows][F + 1] (lam of step 5 as the row's last frame
 *     used it; NaN for a row without frames).  ws: 16-byte aligned.
 * No atomics, no scratch, every sum in an order fixed by the indices: a row's bits depend neither
 * on T, nor on the other rows, nor on the samples past its length.  rows in 1 .. 65535, T in
 * 1 .. 2^24, srate 16000 or 8000; sizes, NULL pointers, dtypes and the alignment of ws are checked
 * before any launch.
 */
#ifndef SEGAN_OMLSA_H
#define SEGAN_OMLSA_H

#ifdef __cplusplus
extern "C" {
#endif

#define SEGAN_OMLSA_U 8
#define SEGAN_OMLSA_V 15
int segan_omlsa_dims(int rows, int T, int srate, long long* out);
int segan_omlsa(const void* x, int x_dtype, const int* lengths, int rows, int T, int srate,
                void* y, int y_dtype, int* nframes, double* presence, int* rough, double* noise,
                void* ws, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGAN_OMLSA_H */
