"""fp64 numpy oracle of the BSS-eval signal-to-distortion ratio with a distortion filter of up to
512 taps (the SDR of bss_eval_sources).  A plain transcription of the
definition; it imports nothing of the project.

`s` is the clean signal, `x` the processed one (any float dtype; all arithmetic is float64):

  1. r[k] = sum_t s[t] s[t+k], d[k] = sum_t s[t] x[t+k], k < n (lags past the length are 0);
  2. c = argmin ||xp - S c||, S[t, k] = s[t-k], xp = x padded with n - 1 zeros: Toeplitz(r) c = d,
     solved by the Levinson recursion; at order m with prediction error E_m <= 2^-40 r[0] the
     recursion stops and c[k] = 0 for k >= m;
  3. st = S c, St = sum st^2, Ee = sum (xp - st)^2;
  4. 10 log10(St / Ee) dB; NaN for an empty signal, r[0] == 0 or St == Ee == 0; else +inf where
     Ee == 0 and -inf where St == 0.
"""
import math

import numpy as np

MAX_TAPS = 512
GUARD = 2.0 ** -40


def correlations(s, x, n):
    """(r, d): the first n lags of the autocorrelation of s and of its cross-correlation with x."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    L = len(s)
    r, d = np.zeros(n), np.zeros(n)
    for k in range(min(n, L)):
        r[k] = np.dot(s[:L - k], s[k:])
        d[k] = np.dot(s[:L - k], x[k:])
    return r, d


def levinson(r, d, guard=GUARD):
    """(c, order): Toeplitz(r) c = d by the Levinson recursion for a general right-hand side.
    `order` is the number of taps solved for: n, or the m at which E_m <= guard * r[0]."""
    r = np.asarray(r, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    n = len(r)
    c, a = np.zeros(n), np.zeros(n)      # a[1 .. m]: the predictor of order m
    E = r[0]
    floor = guard * r[0]
    for m in range(n):
        if m > 0:
            k = -(r[m] + np.dot(a[1:m], r[m - 1:0:-1])) / E
            a[1:m] = a[1:m] + k * a[m - 1:0:-1]
            a[m] = k
            E = E * (1.0 - k * k)
        if not E > floor:
            return c, m
        lam = (d[m] - np.dot(c[:m], r[m:0:-1])) / E
        c[:m] = c[:m] + lam * a[m:0:-1]
        c[m] = lam
    return c, n


def solve_lstsq(r, d):
    """Toeplitz(r) c = d by numpy's SVD least squares: the recursion's cross-check."""
    n = len(r)
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return np.linalg.lstsq(np.asarray(r, dtype=np.float64)[idx], np.asarray(d, dtype=np.float64),
                           rcond=None)[0]


def energies(s, x, c):
    """(St, Ee) of the projection st = c * s and the rest xp - st over t < L + n - 1; the taps are
    applied in ascending order."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    L, n = len(s), len(c)
    if L == 0:
        return 0.0, 0.0
    st = np.zeros(L + n - 1)
    for k in range(n):
        st[k:k + L] += c[k] * s
    e = -st
    e[:L] += x
    return float(np.dot(st, st)), float(np.dot(e, e))


def value(L, r0, St, Ee):
    if L == 0 or r0 == 0.0:
        return math.nan
    if Ee == 0.0:
        return math.nan if St == 0.0 else math.inf
    if St == 0.0:
        return -math.inf
    return 10.0 * math.log10(St / Ee)


def sdr_stages(s, x, taps=MAX_TAPS, solver='levinson'):
    """Every stage of the measure as a dict: r, d, c, order, target_energy, error_energy, sdr."""
    if not 1 <= taps <= MAX_TAPS:
        raise ValueError('taps must lie in 1 .. {}'.format(MAX_TAPS))
    r, d = correlations(s, x, taps)
    if solver == 'levinson':
        c, order = levinson(r, d)
    elif r[0] == 0.0:
        c, order = np.zeros(taps), 0
    else:
        c, order = solve_lstsq(r, d), taps
    St, Ee = energies(s, x, c)
    return {'r': r, 'd': d, 'c': c, 'order': order, 'target_energy': St, 'error_energy': Ee,
            'sdr': value(len(s), r[0], St, Ee)}


def sdr(s, x, taps=MAX_TAPS):
    return sdr_stages(s, x, taps)['sdr']


def sdr_lstsq(s, x, taps=MAX_TAPS):
    """The same value with Toeplitz(r) c = d solved by least squares."""
    return sdr_stages(s, x, taps, solver='lstsq')['sdr']


def sdr_delay_matrix(s, x, taps):
    """The definition itself: least squares on the explicit delay matrix S [L + n - 1, n], no
    correlations.  For small taps only (the matrix is dense)."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    L = len(s)
    S = np.zeros((L + taps - 1, taps))
    for k in range(taps):
        S[k:k + L, k] = s
    xp = np.concatenate([x, np.zeros(taps - 1)])
    c = np.linalg.lstsq(S, xp, rcond=None)[0]
    st = S @ c
    e = xp - st
    return value(L, float(np.dot(s, s)), float(np.dot(st, st)), float(np.dot(e, e)))


def sdr_one_tap(s, x):
    """taps = 1 in closed form: 10 log10(alpha^2 <s,s> / <e,e>), alpha = <s,x> / <s,s>,
    e = x - alpha s (SI-SDR without the mean removal)."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    ss = float(np.dot(s, s))
    if len(s) == 0 or ss == 0.0:
        return math.nan
    alpha = float(np.dot(s, x)) / ss
    e = x - alpha * s
    return value(len(s), ss, alpha * alpha * ss, float(np.dot(e, e)))
