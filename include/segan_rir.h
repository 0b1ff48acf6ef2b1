/*
 * segan_rir.h — extension header of libsegan_hip.so: room impulse responses of shoebox rooms by
 * the image-source method.
 *
 * The exports below are purely additive: SEGAN_ABI_VERSION stays 17, and include/segan_hip.h,
 * include/segan_dereverb.h, include/segan_pyin.h and include/segan_omlsa.h are unchanged.  The
 * conventions are the main header's (`stream` a hipStream_t as void*, 0 on success, negative on
 * error with the message in segan_last_error(), here prefixed `rir:`); the binding reads this file
 * with the same reader (segan_pytorch_amd/_lib.py: RIR_SIGNATURES, RIR_DEFINES).
 *
 * The image-source method (Allen & Berkley 1979) with Peterson's windowed-sinc impulse for the
 * fractional delays, defined by scripts/rir_oracle.py.  All arithmetic is fp64, every product and
 * sum rounded on its own.  Per response: room L[3] in metres, source s[3], receiver r[3], beta[6]
 * (walls x = 0, x = Lx, y = 0, y = Ly, z = 0, z = Lz), c = 343 m/s, Hw = srate / 250.
 *   Image (n, l, m) in Z^3, (q, j, k) in {0, 1}^3:
 *     px = ((1 - 2 q) sx - rx) + (2 n) Lx, py and pz alike; d = sqrt((px^2 + py^2) + pz^2);
 *     tau = d (srate / c);
 *     a = (((tx0[|n - q|] tx1[|n|]) (ty0[|l - j|] ty1[|l|])) (tz0[|m - k|] tz1[|m|])) / ((4 pi) d)
 *     with the power tables t_w[i] = beta_w^i that the caller built (t_w[0] = 1,
 *     t_w[i] = t_w[i - 1] beta_w).
 *   With n0 = floor(tau), f = tau - n0, sample t = n0 + k' (0 <= t < the row's length) receives,
 *     for |k' - f| < Hw, (a (0.5 (1 + cos(pi (k' - f) / Hw)))) sinc with
 *     sinc = -(-1)^k' sin(pi f) / (pi (k' - f)), 1 where k' - f = 0.  The cosine is taken by the
 *     angle-addition identity from a host-built table of (cos, sin)(pi k' / Hw).
 *   The images of a row: those with n0 - Hw + 1 <= length - 1, whatever their amplitude.
 *   segan_rir_dims (host only): out[4] = {Hw, the stride of the power tables (entries per wall:
 *     enough for rooms of 1 m), the tiles of SEGAN_RIR_TILE samples of a row, the bytes of
 *     workspace `ws` for `count` responses}.
 *   segan_rir: geom fp64 [count][SEGAN_RIR_GEOM] = L, s, r, beta on the HOST (checked, then copied
 *     into ws in stream order; the call returns after the copy has been read); tables fp64
 *     [count][6][stride] (device); lengths int[count] (device; NULL: all T; clamped to 0 .. T);
 *     h fp64 [count][T] (device), zero from the row's length on; images long long[count] (device,
 *     optional); ws: 8-byte aligned.
 * One workgroup per (tile, response), one thread per sample, the sample in a register; the
 * workgroup enumerates the images that can reach its tile in an order fixed by their indices and
 * every thread decides by its own test |k' - f| < Hw.  No atomics, no scratch: the bits of sample t
 * of a response depend neither on count, nor on the other rows, nor on T, nor on lengths beyond the
 * masking.  count in 1 .. 65535, T in 1 .. 2^20, srate 16000 or 8000, L in [1, 50] m per axis,
 * s and r strictly inside the room and at least 0.05 m apart, beta in [0, 1]; sizes, NULL pointers,
 * alignment and the geometry are checked before any launch.
 */
#ifndef SEGAN_RIR_H
#define SEGAN_RIR_H

#ifdef __cplusplus
extern "C" {
#endif

#define SEGAN_RIR_TILE 256
#define SEGAN_RIR_GEOM 15
#define SEGAN_RIR_MAX_T 1048576
int segan_rir_dims(int count, int T, int srate, long long* out);
int segan_rir(const double* geom, const double* tables, const int* lengths, int count, int T,
              int srate, double* h, long long* images, void* ws, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SEGAN_RIR_H */
