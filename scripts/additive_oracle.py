"""fp64 numpy oracle of the additive-noise mixer: the ITU-T P.56 method-B
active speech level and the SNR mix of the reference's `Additive` (segan/utils.py:43-297), restated
without its per-sample python loop.

    asl_p56(x, srate)          -> dict(sq, asl_ms, asl, c0 (None where the reference returns None),
                                       counts, q, status)
    mix(clean, segment, snr, Px) -> dict(noisy (fp64), noisy32, Pn, sf, n)

The hangover loop (utils.py:206-215, with its `break`) counts, per threshold c_j, the samples k for
which some k' in [k - I, k] has q[k'] >= c_j: the exceedance set dilated I samples to the right.
`activity_counts` computes that from a running maximum of the last exceeding index;
`activity_counts_loop` is the literal loop, kept to check the equivalence on short signals.
Everything else (finalisation, bin_interp with its `(midcount - lwcount) / 2` branch and the 10 %
tolerance relaxation) follows the reference line by line; the only addition is an iteration cap in
bin_interp, reported as status 1, where the reference would spin (NaN input).
"""
import math

import numpy as np
from scipy.signal import lfilter

T_SMOOTH = 0.03      # envelope time constant, s
H_HANG = 0.2         # hangover, s
MARGIN = 15.9        # dB
EPS = 1e-22
INTERP_CAP = 1000
CLIP_CAP = 1000


def thresholds(nbits=16):
    return 2.0 ** np.arange(-15, nbits - 16, dtype=np.float64)


def hangover(srate):
    return int(np.ceil(srate * H_HANG))


def envelope(x, srate):
    """q of utils.py:201-204 in float64."""
    g = np.exp(-1 / (srate * T_SMOOTH))
    xa = np.abs(np.asarray(x, dtype=np.float64))
    p = lfilter(np.ones(1) - g, np.array([1, -g]), xa)
    return lfilter(np.ones(1) - g, np.array([1, -g]), p)


def activity_counts(q, srate, nbits=16):
    """a_j = #{k : exists k' in [k - I, k] with q[k'] >= c_j}, int64 [nbits - 1]."""
    I = hangover(srate)
    k = np.arange(len(q))
    out = np.zeros(nbits - 1, dtype=np.int64)
    for j, c in enumerate(thresholds(nbits)):
        last = np.maximum.accumulate(np.where(q >= c, k, -1)) if len(q) else k
        out[j] = int(np.count_nonzero((last >= 0) & (k - last <= I)))
    return out


def activity_counts_loop(q, srate, nbits=16):
    """The reference's loop, utils.py:194-215, as written."""
    c = thresholds(nbits)
    I = np.ceil(srate * H_HANG)
    a = np.zeros(c.shape[0])
    hang = np.ones(c.shape[0]) * I
    for k in range(len(q)):
        for j in range(nbits - 1):
            if q[k] >= c[j]:
                a[j] = a[j] + 1
                hang[j] = 0
            elif hang[j] < I:
                a[j] = a[j] + 1
                hang[j] = hang[j] + 1
            else:
                break
    return a.astype(np.int64)


def bin_interp(upcount, lwcount, upthr, lwthr, margin, tol, trace=None):
    """utils.py:255-297.  Returns (asl_ms_log, cc, status); `trace` collects |quantity - bound| of
    every comparison made, for the fixture's knife-edge check."""
    def note(val, bound):
        if trace is not None:
            trace.append(abs(abs(val) - bound))

    if tol < 0:
        tol = -tol
    iterno = 1
    note(upcount - upthr - margin, tol)
    if abs(upcount - upthr - margin) < tol:
        return lwcount, lwthr, 0
    note(lwcount - lwthr - margin, tol)
    if abs(lwcount - lwthr - margin) < tol:
        return lwcount, lwthr, 0
    midcount = (upcount + lwcount) / 2
    midthr = (upthr + lwthr) / 2
    status = 0
    while True:
        diff = midcount - midthr - margin
        note(diff, tol)
        if abs(diff) <= tol:
            break
        iterno += 1
        if iterno > INTERP_CAP:
            status = 1
            break
        if iterno > 20:
            tol *= 1.1
        note(diff, tol)
        if diff > tol:
            midcount = (upcount + midcount) / 2
            midthr = (upthr + midthr) / 2
        elif diff < -tol:
            midcount = (midcount - lwcount) / 2
            midthr = (midthr + lwthr) / 2
    return midcount, midthr, status


def finalise(sq, a, x_len, nbits=16, trace=None):
    """utils.py:216-253: (asl_ms, asl, c0, status) from the energy, the counts and the length."""
    c = thresholds(nbits)
    asl, asl_ms, c0, status = 0, 0, None, 0
    if a[0] == 0:
        return asl_ms, asl, c0, status
    AdB1 = 10 * np.log10(sq / float(a[0]) + EPS)
    CdB1 = 20 * np.log10(c[0] + EPS)
    if trace is not None:
        trace.append(abs(AdB1 - CdB1 - MARGIN))
    if AdB1 - CdB1 < MARGIN:
        return asl_ms, asl, c0, status
    AdB = np.zeros(c.shape[0])
    CdB = np.zeros(c.shape[0])
    AdB[0], CdB[0] = AdB1, CdB1
    for j in range(1, AdB.shape[0]):
        AdB[j] = 10 * np.log10(sq / (float(a[j]) + EPS) + EPS)
        CdB[j] = 20 * np.log10(c[j] + EPS)
    for j in range(1, AdB.shape[0]):
        if a[j] != 0:
            delta = AdB[j] - CdB[j]
            if trace is not None:
                trace.append(abs(delta - MARGIN))
            if delta <= MARGIN:
                asl_ms_log, cl0, status = bin_interp(AdB[j], AdB[j - 1], CdB[j], CdB[j - 1],
                                                     MARGIN, 0.5, trace)
                asl_ms = 10 ** (asl_ms_log / 10)
                asl = (sq / x_len) / asl_ms
                c0 = 10 ** (cl0 / 20)
                break
    return asl_ms, asl, c0, status


def asl_p56(x, srate=16000, nbits=16, trace=None):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    sq = float(np.dot(x, x))
    q = envelope(x, srate)
    a = activity_counts(q, srate, nbits)
    asl_ms, asl, c0, status = finalise(sq, a, x.shape[0], nbits, trace)
    return dict(sq=sq, asl_ms=float(asl_ms), asl=float(asl), c0=None if c0 is None else float(c0),
                counts=a, q=q, status=status)


def threshold_margin(q, nbits=16):
    """min |q[k] - c_j| / c_j over all k, j."""
    if len(q) == 0:
        return math.inf
    return min(float(np.min(np.abs(q - c)) / c) for c in thresholds(nbits))


def clip_divisions(mx, mn):
    """Number of divisions of the anti-clipping loop (utils.py:89-95) run on a row's (max, min)."""
    n, small = 0, 0.1
    while (mx >= 1 or mn < -1) and n < CLIP_CAP:
        mx, mn = mx / (1. + small), mn / (1. + small)
        small = small + 0.1
        n += 1
    return n


def mix(clean, segment, snr_db, Px, prev=None):
    """utils.py:125-132 and 89-95 in float64.  Px == 0 gives sf = 0; Pn == 0 is defined as sf = 0
    (the reference divides by zero).  prev = (clean sample, noise sample) preceding the row."""
    clean = np.asarray(clean, dtype=np.float64)
    seg = np.asarray(segment, dtype=np.float64)
    Pn = float(np.dot(seg, seg) / clean.shape[0])
    sf = float(np.sqrt(Px / Pn / (10 ** (float(snr_db) / 10)))) if Pn > 0 else 0.0
    noisy = clean + seg * sf
    n = clip_divisions(noisy.max(), noisy.min()) if noisy.size and not np.isnan(noisy).any() else 0
    pv = None if prev is None else np.float64(prev[0]) + np.float64(prev[1]) * sf
    small = 0.1
    for _ in range(n):
        noisy = noisy / (1. + small)
        if pv is not None:
            pv = pv / (1. + small)
        small = small + 0.1
    out = dict(noisy=noisy, noisy32=noisy.astype(np.float32), Pn=Pn, sf=sf, n=n)
    if pv is not None:
        out['prev32'] = np.float32(pv)
    return out
