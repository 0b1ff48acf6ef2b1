"""fp64 numpy oracle of three objective measures: the frequency-weighted
segmental SNR (fwSNRseg) and the LPC cepstrum distance (CD) of Hu & Loizou's evaluation, and the
scale-invariant SDR of Le Roux et al. (2019).  A plain transcription of the definitions; it imports
nothing of the project.

`s` is the clean signal, `x` the processed one (any float dtype; all arithmetic is float64).
"""
import math

import numpy as np

ALPHA = 0.95
NCRIT = 25
CENT_FREQ = (50., 120, 190, 260, 330, 400, 470, 540, 617.372, 703.378, 798.717, 904.128, 1020.38,
             1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97,
             2978.04, 3276.17, 3597.63)
BANDWIDTH = (70., 70, 70, 70, 70, 70, 70, 77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
             140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072,
             298.126, 321.465, 346.136)
ERR_FLOOR = 2.0 ** -52
CD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)


def geometry(srate):
    """(win, hop, nfft, P): the 30 ms window, its quarter, the DFT size and the LPC order."""
    win = int(round(30.0 * srate / 1000.0))
    nfft = int(2 ** math.ceil(math.log(2 * win) / math.log(2)))
    return win, win // 4, nfft, (16 if srate >= 10000 else 10)


def frame_count(n, srate):
    win, hop = geometry(srate)[:2]
    if n <= 0 or hop <= 0:
        return 0
    return max(int(n / hop - win / hop), 0)


def window(win):
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, win + 1) / (win + 1)))


def frames(sig, srate):
    """The windowed frames [nf, win] of a signal."""
    win, hop = geometry(srate)[:2]
    sig = np.asarray(sig, dtype=np.float64)
    nf = frame_count(len(sig), srate)
    w = window(win)
    return np.stack([sig[f * hop:f * hop + win] * w for f in range(nf)]) if nf else \
        np.zeros((0, win))


def crit_filters(srate):
    """[25, nfft/2]: Gaussian critical-band filters with their norm factor, zeroed below -30 dB."""
    nfft = geometry(srate)[2]
    half = nfft // 2
    max_freq = srate / 2.0
    min_factor = math.exp(-30.0 / (2 * 2.303))
    j = np.arange(half, dtype=np.float64)
    crit = np.zeros((NCRIT, half))
    for i in range(NCRIT):
        f0 = math.floor((CENT_FREQ[i] / max_freq) * half)
        bw = (BANDWIDTH[i] / max_freq) * half
        norm = math.log(BANDWIDTH[0]) - math.log(BANDWIDTH[i])
        u = (j - f0) / bw
        v = np.exp(-11 * (u * u) + norm)
        crit[i] = np.where(v > min_factor, v, 0.0)
    return crit


def fwsegsnr_bands(s, x, srate):
    """(ce, pe) [nf, 25]: the band values of the normalised magnitude spectra."""
    nfft = geometry(srate)[2]
    half = nfft // 2
    crit = crit_filters(srate)
    with np.errstate(all='ignore'):
        C = np.abs(np.fft.fft(frames(s, srate), nfft, axis=1))[:, :half]
        X = np.abs(np.fft.fft(frames(x, srate), nfft, axis=1))[:, :half]
        Cn = C / C.sum(axis=1, keepdims=True)
        Xn = X / X.sum(axis=1, keepdims=True)
    return Cn @ crit.T, Xn @ crit.T


def fwsegsnr_frames(s, x, srate=16000, clip=True):
    """Per-frame fwSNRseg [nf]: NaN where the value is not finite."""
    ce, pe = fwsegsnr_bands(s, x, srate)
    with np.errstate(all='ignore'):
        err = np.maximum((ce - pe) ** 2, ERR_FLOOR)
        W = ce ** 0.2
        snr = 10.0 * np.log10(ce ** 2 / err)
        v = (W * snr).sum(axis=1) / W.sum(axis=1)
    fin = np.isfinite(v)
    if clip:
        v = np.clip(v, -10.0, 35.0)
    return np.where(fin, v, np.nan)


def finite_mean(v):
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(v.mean()) if v.size else math.nan


def fwsegsnr(s, x, srate=16000):
    return finite_mean(fwsegsnr_frames(s, x, srate))


def lags(frame, P, order='forward', dtype=np.float64):
    """R[0..P] of one windowed frame.  `order` ('forward' / 'reversed': the products summed from
    the first or from the last) and `dtype` exist for the sensitivity measurement."""
    fr = np.asarray(frame, dtype=dtype)
    if order == 'reversed':
        fr = np.ascontiguousarray(fr[::-1])
    return np.array([np.dot(fr[:len(fr) - j], fr[j:]) for j in range(P + 1)], dtype=dtype)


def levinson(R):
    """[1, a_1 .. a_P], the prediction polynomial, by Levinson-Durbin in R's dtype."""
    P = len(R) - 1
    one = R.dtype.type(1)
    a = np.ones(P, dtype=R.dtype)
    E = R[0]
    with np.errstate(all='ignore'):
        for i in range(P):
            acc = R.dtype.type(0)
            for j in range(i):
                acc = acc + a[j] * R[i - j]
            rc = (R[i + 1] - acc) / E
            prev = a.copy()
            for j in range(i):
                a[j] = prev[j] - rc * prev[i - 1 - j]
            a[i] = rc
            E = (one - rc * rc) * E
    return np.concatenate([[one], -a]).astype(R.dtype)


def cepstrum(A):
    """c[1..P] of A = [1, a_1 .. a_P]: c_1 = -a_1, c_n = -a_n - (1/n) sum_{k<n} k c_k a_{n-k}."""
    P = len(A) - 1
    c = np.zeros(P + 1, dtype=A.dtype)
    c[1] = -A[1]
    for n in range(2, P + 1):
        acc = A.dtype.type(0)
        for k in range(1, n):
            acc = acc + k * c[k] * A[n - k]
        c[n] = -A[n] - acc / n
    return c[1:]


def cd_frames(s, x, srate=16000, order='forward', dtype=np.float64):
    """Per-frame cepstrum distance [nf] (float64): NaN where either frame has R[0] == 0."""
    P = geometry(srate)[3]
    fs, fx = frames(s, srate), frames(x, srate)
    out = np.full(len(fs), np.nan)
    for f in range(len(fs)):
        Rs, Rx = lags(fs[f], P, order, dtype), lags(fx[f], P, order, dtype)
        if Rs[0] == 0 or Rx[0] == 0:
            continue
        d = cepstrum(levinson(Rs)) - cepstrum(levinson(Rx))
        acc = dtype(0)
        for v in d:
            acc = acc + v * v
        out[f] = min(10.0, CD_SCALE * float(np.sqrt(acc)))
    return out


def trimmed_count(n, alpha=ALPHA):
    return int(round(n * alpha))


def trimmed_mean(v):
    """The 0.95-trimmed mean of the finite values (NaN without any)."""
    v = np.asarray(v, dtype=np.float64)
    v = np.sort(v[np.isfinite(v)])
    return float(v[:trimmed_count(v.size)].mean()) if v.size else math.nan


def cepstral_distance(s, x, srate=16000):
    return trimmed_mean(cd_frames(s, x, srate))


def si_sdr(s, x):
    """10 log10(alpha^2 <s,s> / <e,e>), both means removed, e = alpha s - x summed sample by
    sample: NaN where <s,s> is 0, +inf where <e,e> is."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    s = s - s.mean()
    x = x - x.mean()
    ss = float(np.dot(s, s))
    if ss == 0:
        return math.nan
    alpha = float(np.dot(s, x)) / ss
    e = alpha * s - x
    ee = float(np.dot(e, e))
    if ee == 0:
        return math.inf
    return 10.0 * math.log10(alpha * alpha * ss / ee)


def si_sdr_moments(s, x):
    """si_sdr with the means and alpha taken from the raw moments (sum s, sum x, sum s s,
    sum s x) of one pass, as the kernel takes them; <s,s> and <e,e> from the centred samples."""
    s = np.asarray(s, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    n = float(len(s))
    S, X, SS, SX = s.sum(), x.sum(), np.dot(s, s), np.dot(s, x)
    with np.errstate(all='ignore'):
        alpha = (SX - S * X / n) / (SS - S * S / n)
        sc = s - S / n
        e = alpha * sc - (x - X / n)
        ss, ee = float(np.dot(sc, sc)), float(np.dot(e, e))
        if not ss > 0:
            return math.nan
        return math.inf if ee == 0 else 10.0 * math.log10(alpha * alpha * ss / ee)
