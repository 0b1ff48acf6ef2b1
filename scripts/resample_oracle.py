"""fp64 numpy oracle of the sample-rate conversion behind ops.resample (DESIGN.md section 12
states the rules it follows).  scripts/make_golden_resample.py runs it to write
tests/golden/resample.pt, and the tests run it again.  Importable on its own (numpy).

    import resample_oracle as R
    y = R.convert(x, 48000, 16000)                    # fp64, ceil(len(x) / 3) samples
    y16, nclip = R.to_int16(R.convert(x16, 48000, 16000))

The filter is scipy.signal.resample_poly's with a Kaiser window: (zeros, beta) = (10, 5.0) is
scipy's default; the package's default is (32, 8.6)."""
import math

import numpy as np

ZEROS, BETA = 32, 8.6
SCIPY_ZEROS, SCIPY_BETA = 10, 5.0
RATE_MIN, RATE_MAX = 4000, 192000
ZEROS_MAX, BETA_MAX, MX_MAX = 64, 20.0, 4096


def ratio(rate_in, rate_out):
    """(p, q) = rate_out / rate_in in lowest terms."""
    rate_in, rate_out = int(rate_in), int(rate_out)
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def design(p, q, zeros, beta):
    """The taps of p / q: mx = max(p, q), lh = zeros mx, h[t] = sinc(t / mx) kaiser(2 lh + 1, beta)[t + lh]
    for t = -lh .. lh, G[t + lh] = p h[t] / sum(h).  p == q: [1.0]."""
    if p == q:
        return np.ones(1)
    mx = max(p, q)
    lh = int(zeros) * mx
    t = np.arange(-lh, lh + 1)
    h = np.sinc(t / mx) * np.kaiser(2 * lh + 1, beta)
    return p * h / np.sum(h)


def plan(rate_in, rate_out, zeros=ZEROS, beta=BETA):
    """(p, q, taps) of a conversion within the public limits: design(p, q, zeros, beta).  Equal
    rates: (1, 1, [1.0])."""
    for r in (rate_in, rate_out):
        if not RATE_MIN <= int(r) <= RATE_MAX:
            raise ValueError('rate {} outside {} .. {} Hz'.format(r, RATE_MIN, RATE_MAX))
    if not 1 <= int(zeros) <= ZEROS_MAX or not 0.0 <= beta <= BETA_MAX:
        raise ValueError('zeros {} outside 1 .. {} or beta {} outside 0 .. {}'.format(
            zeros, ZEROS_MAX, beta, BETA_MAX))
    p, q = ratio(rate_in, rate_out)
    if max(p, q) > MX_MAX:
        raise ValueError('{} -> {} Hz reduces to {} / {}: max(p, q) above {}'.format(
            rate_in, rate_out, p, q, MX_MAX))
    return p, q, design(p, q, zeros, beta)


def out_len(L, p, q):
    return -(-int(L) * p // q)


def resample(x, p, q, taps):
    """y[m] = sum_n x[n] G[m q - n p] over |m q - n p| <= lh, 0 <= n < Lx (ascending n),
    m = 0 .. ceil(Lx p / q) - 1; fp64."""
    x = np.asarray(x, dtype=np.float64)
    Lx = len(x)
    Ly = out_len(Lx, p, q)
    lh = (len(taps) - 1) // 2
    c = np.arange(Ly, dtype=np.int64) * q
    n_lo = np.maximum(-((lh - c) // p), 0)          # ceil((c - lh) / p), at least 0
    n_hi = np.minimum((c + lh) // p, Lx - 1)
    y = np.zeros(Ly)
    for j in range(2 * lh // p + 2):
        n = n_lo + j
        ok = n <= n_hi
        if not ok.any():
            break
        nn = np.where(ok, n, 0)
        y += np.where(ok, x[nn] * taps[np.where(ok, c - nn * p + lh, 0)], 0.0)
    return y


def convert(x, rate_in, rate_out, zeros=ZEROS, beta=BETA):
    """x (any real dtype, int16 values used as they are) at rate_in -> fp64 at rate_out."""
    p, q, taps = plan(rate_in, rate_out, zeros, beta)
    return resample(x, p, q, taps)


def to_int16(y):
    """Round half to even, saturate to -32768 .. 32767: (int16 array, saturated samples)."""
    r = np.rint(np.asarray(y, dtype=np.float64))
    clip = (r > 32767) | (r < -32768)
    return np.clip(r, -32768, 32767).astype(np.int16), int(clip.sum())


def half_distance(y):
    """The smallest distance of any value of y to a half-integer (where rounding could flip)."""
    y = np.asarray(y, dtype=np.float64)
    if y.size == 0:
        return np.inf
    return float(np.abs(y - np.floor(y) - 0.5).min())


def convert_int16(x, rate_in, rate_out, zeros=ZEROS, beta=BETA):
    """int16 (or any) samples -> (int16 at rate_out, saturated samples)."""
    return to_int16(convert(x, rate_in, rate_out, zeros, beta))


def resample_scipy(x, p, q, taps):
    """The same conversion by scipy.signal.resample_poly with the oracle's taps as its window."""
    from scipy.signal import resample_poly
    x = np.asarray(x, dtype=np.float64)
    if p == 1 and q == 1:
        return x.copy()
    return resample_poly(x, p, q, window=np.asarray(taps) / p)
