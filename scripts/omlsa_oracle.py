"""The numpy oracle of the OM-LSA enhancer with IMCRA noise tracking: the
definition that segan_omlsa.hip, ops.omlsa_rows and baselines.omlsa implement.

The optimally-modified log-spectral-amplitude estimator (Cohen & Berdugo, Signal Processing 81,
2001) with the noise spectrum of the improved minima-controlled recursive averaging (Cohen, IEEE
Trans. SAP 11, 2003), written from the two papers.  It needs no leading noise segment: the noise
spectrum follows the minima of the smoothed periodogram over a sliding window of U V frames, so
it keeps adapting after the level of the noise has changed, where the VAD-gated estimate of
scripts/denoise_oracle.py stops for good.  The gain is weighted with IMCRA's own speech-presence
probability p; Cohen's separate local / global / frame prior for the gain is not part of it.

Framing, window, analysis and synthesis are section 20's (scripts/denoise_oracle.py, imported
here): F = srate / 50, H = F / 2, N = 2 F, the Hamming window scaled by H / sum w, nf = L // H - 1
frames for L >= 6 F and none below (the row is then returned unchanged), spectrum S_t[k] of frame
t at the bins k = 0 .. F with s2 = re^2 + im^2, and the overlap-add of the first F samples of the
inverse DFT, the earlier frame added first, zeros from (nf + 1) H on.

sm3(a)[k] = (0.25 a[k - 1] + 0.5 a[k]) + 0.25 a[k + 1] with a[-1] := a[1] and a[F + 1] := a[F - 1]
(the Hermitian mirror).  Per frame t, elementwise over k, every product and sum rounded on its own:

   1. Sf = sm3(s2); S = Sf (t = 0) or as S + (1 - as) Sf; Smin = Smact = S and all U history slots
      = S (t = 0), else Smin = min(Smin, S), Smact = min(Smact, S).
   2. th = Bmin Smin; I = (s2 < g0 th) and (S < z0 th): the rough decision "no speech here".
   3. den = sm3(I), num = sm3(I s2); Stf = num / den where den > 0, else the previous St (Sf at
      t = 0); St = Stf (t = 0) or as St + (1 - as) Stf; Stmin, Stmact and a second history as in 1.
   4. tth = Bmin Stmin; low = St < z0 tth; q = 1 where low and s2 <= tth; q = (g1 - s2 / tth) /
      (g1 - 1) where low and s2 < g1 tth; q = 0 otherwise: the a-priori speech absence.
   5. lam = max(beta lbar, 2^-100) with lbar = s2 of frame 0 at t = 0; gamma = min(s2 / lam, 40);
      xi = max((a P) / lam + (1 - a) max(gamma - 1, 0), 10^-2.5), the first term a at t = 0;
      A = xi / (1 + xi); nu = A gamma.
   6. p = 0 where q = 1, p = 1 where q = 0, else 1 / (1 + ((q / (1 - q)) (1 + xi)) exp(-nu)).
   7. at = ad + (1 - ad) p; lbar <- at lbar + (1 - at) s2, after gamma and xi of this frame.
   8. GH1 = A exp(E1(max(nu, 2^-40)) / 2); G = exp(p ln GH1 + (1 - p) ln Gmin); P <- (GH1 GH1) s2.
   9. If (t + 1) % V == 0: slot j = ((t + 1) / V - 1) % U; history[j] <- Smact; Smin <- the minimum
      over the U slots; Smact <- S; the same for the second history.
  10. presence_t = vad_sum(p) / 2 (the c_k-weighted mean of p in section 20's groups-of-64 order);
      rough_t = the number of bins with I = 1.

as = 0.9, ad = 0.85, a = 0.92, beta = 1.47, Bmin = 1.66, g0 = 4.6, g1 = 3, z0 = 1.67, U = 8,
V = 15, ln Gmin = ln 10^(-25/20) as the one literal LN_GMIN.

Like scripts/denoise_oracle.py the whole oracle runs unchanged in numpy.longdouble (`dtype=`): the
movement between the two runs is what the tolerances of the GPU tests are made of
(scripts/make_golden_omlsa.py).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_oracle as D  # noqa: E402

RATES = D.RATES
ALPHA_S = 0.9                # smoothing of the periodogram, both iterations
ALPHA_D = 0.85               # smoothing of the noise spectrum
ALPHA = 0.92                 # decision-directed weight
BETA = 1.47                  # bias of the noise spectrum
B_MIN = 1.66                 # bias of the minimum
GAMMA0 = 4.6
GAMMA1 = 3.0
ZETA0 = 1.67
U = 8                        # slots of the minimum window
V = 15                       # frames per slot
LN_GMIN = -2.878231366242557           # ln 10^(-25/20)
XI_MIN = D.XI_MIN
GAMMA_MAX = D.GAMMA_MAX
LAMBDA_MIN = D.LAMBDA_MIN
E1_MIN = D.E1_MIN

constants = D.constants
n_frames = D.n_frames


def sm3(a, dtype=np.float64):
    """The three-tap smoothing over the bins with the Hermitian mirror at both ends."""
    lo = np.concatenate([a[1:2], a[:-1]])
    hi = np.concatenate([a[1:], a[-2:-1]])
    return (dtype(0.25) * lo + dtype(0.5) * a) + dtype(0.25) * hi


def _rel(a, b):
    """The smallest |a - b| / max(a, b) over the pairs with max(a, b) > 0 (inf without one)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    m = np.maximum(a, b)
    ok = m > 0
    return float(np.min(np.abs(a - b)[ok] / m[ok])) if ok.any() else np.inf


class _Minimum:
    """Steps 1 / 3 / 9 for one smoothed periodogram: its value, the two running minima and the U
    slots of the window."""

    def __init__(self):
        self.s = None

    def smooth(self, f, a, b):
        if self.s is None:
            self.s = f
            self.min = self.mact = f
            self.hist = [f] * U
        else:
            self.s = a * self.s + b * f
            self.min = np.minimum(self.min, self.s)
            self.mact = np.minimum(self.mact, self.s)
        return self.s

    def roll(self, t):
        if (t + 1) % V == 0:
            self.hist[((t + 1) // V - 1) % U] = self.mact
            m = self.hist[0]
            for h in self.hist[1:]:
                m = np.minimum(m, h)
            self.min = m
            self.mact = self.s


def omlsa(x, srate=16000, dtype=np.float64):
    """One row x [L] -> dict: 'y' [L] (dtype), 'nframes', 'presence' [nf] (the weighted mean of p
    over the bins), 'rough' [nf] (int: bins the rough decision of step 2 called noise), 'noise'
    [F + 1] (lam of step 5 as the last frame used it; empty without a frame), 'margin' (the
    smallest relative distance of the three discontinuous comparisons of steps 2 and 4 over
    every bin and frame; inf without one)."""
    F, H, N = constants(srate)
    x = np.asarray(x).astype(dtype)
    L = len(x)
    nf = n_frames(L, srate)
    if nf == 0:
        return {'y': x.copy(), 'nframes': 0, 'presence': np.zeros(0, dtype),
                'rough': np.zeros(0, np.int64), 'noise': np.zeros(0, dtype), 'margin': np.inf}
    one = dtype(1)
    a_s, a_d, a = dtype(ALPHA_S), dtype(ALPHA_D), dtype(ALPHA)
    b_s, b_d, b = one - a_s, one - a_d, one - a
    bmin, g0, g1, z0 = dtype(B_MIN), dtype(GAMMA0), dtype(GAMMA1), dtype(ZETA0)
    w = D.window(F, dtype)
    C, S, Ci, Si = D.dft_tables(F, dtype)
    y = np.zeros(L, dtype)
    presence = np.zeros(nf, dtype)
    rough = np.zeros(nf, np.int64)
    first, second = _Minimum(), _Minimum()
    margin = np.inf
    lbar = P = lam = None
    for t in range(nf):
        seg = w * x[t * H:t * H + F]
        re, im = C @ seg, -(S @ seg)
        s2 = re * re + im * im
        # 1, 2
        sf = sm3(s2, dtype)
        s = first.smooth(sf, a_s, b_s)
        th = bmin * first.min
        ind = (s2 < g0 * th) & (s < z0 * th)
        margin = min(margin, _rel(s2, g0 * th), _rel(s, z0 * th))
        # 3
        i1 = ind.astype(dtype)
        den, num = sm3(i1, dtype), sm3(i1 * s2, dtype)
        prev = sf if second.s is None else second.s
        with np.errstate(divide='ignore', invalid='ignore'):
            stf = np.where(den > 0, num / den, prev)
        st = second.smooth(stf, a_s, b_s)
        # 4
        tth = bmin * second.min
        low = st < z0 * tth
        margin = min(margin, _rel(st, z0 * tth))
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(low & (s2 < g1 * tth), (g1 - s2 / tth) / (g1 - one), dtype(0))
        q = np.where(low & (s2 <= tth), one, q)
        # 5
        if lbar is None:
            lbar = s2
        lam = np.maximum(dtype(BETA) * lbar, dtype(LAMBDA_MIN))
        gam = np.minimum(s2 / lam, dtype(GAMMA_MAX))
        head = np.full(F + 1, a) if P is None else (a * P) / lam
        xi = np.maximum(head + b * np.maximum(gam - one, dtype(0)), dtype(XI_MIN))
        A = xi / (one + xi)
        nu = A * gam
        # 6
        mid = (q > 0) & (q < 1)
        qm = np.where(mid, q, dtype(0.5))
        p = one / (one + ((qm / (one - qm)) * (one + xi)) * np.exp(-nu))
        p = np.where(q == 1, dtype(0), np.where(q == 0, one, p))
        # 7
        at = a_d + b_d * p
        lbar = at * lbar + (one - at) * s2
        # 8
        gh1 = A * np.exp(D.exp1(np.maximum(nu, dtype(E1_MIN)), dtype) / dtype(2))
        G = np.exp(p * np.log(gh1) + (one - p) * dtype(LN_GMIN))
        P = (gh1 * gh1) * s2
        # 9
        first.roll(t)
        second.roll(t)
        # 10
        presence[t] = D.vad_sum(p, F, dtype) / dtype(2)
        rough[t] = int(ind.sum())
        o = (Ci @ (G * re) - Si @ (G * im)) / dtype(N)
        y[t * H:t * H + F] += o
    return {'y': y, 'nframes': nf, 'presence': presence, 'rough': rough, 'noise': lam,
            'margin': margin}
