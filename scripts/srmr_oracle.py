"""The specification of SRMR, the speech-to-reverberation modulation energy ratio (Falk, Zheng and
Chan 2010), in fp64 numpy / scipy: what segan_srmr (segan_pytorch_amd/csrc/segan_srmr.hip,
DESIGN.md section 16) is tested against.  The time-domain measure of the authors' toolbox: 23
gammatone channels, 8 modulation bands, no energy normalisation ("norm" off); the "fast"
gammatonegram variant is not covered.

One float32 row x of N samples at fs (16000 or 8000), everything in fp64:

  1. centre frequencies cf_i, i = 1 .. 23, on Slaney's ERB scale from fs / 2 down to 125 Hz;
  2. gammatone channel i: four cascaded biquads (Slaney's MakeERBFilters), the first one divided
     by the cascade's magnitude at cf_i, run from zero state in the order +(3+), -(3+), +(3-),
     -(3-) of their numerators;
  3. envelope e_i = |analytic(y_i)|, the analytic signal taken on the row zero-padded to L, the
     smallest power of two >= N (`exact=True`: on exactly N samples, as the toolbox does);
  4. modulation bank: 8 second-order band-passes, centres 4 * 32^(k/7) Hz, Q = 2, zero state;
  5. E[i, k, f] = sum (w m_ik)^2 over frames of wl = ceil(0.256 fs) samples, wi = ceil(0.064 fs)
     apart, full frames only, w the periodic Hamming window; Ebar[i, k] the mean over frames;
  6. BW = ERB of the first channel (from the lowest cf upwards) at which the cumulated share of
     sum_k Ebar[i, k] exceeds 90 %; K* = 5 .. 8 from BW against the bands' left cutoffs (K* = 5
     where BW <= c_4, which the toolbox leaves undefined);
  7. SRMR = sum_i sum_{k<4} Ebar / sum_i sum_{4<=k<K*} Ebar; NaN for N < wl or zero total energy.

`dtype=numpy.longdouble` runs the filters and the sums in extended precision (the transforms stay
fp64): the fixture records the gap between the two as the oracle's own error.
"""
import math

import numpy as np
from scipy.signal import lfilter

CHANNELS = 23
BANDS = 8
EARQ = 9.26449
MINBW = 24.7
LOW_FREQ = 125.0
RATES = (8000, 16000)


def centre_freqs(fs):
    """The 23 centre frequencies, descending from just below fs / 2 to 125 Hz."""
    high = fs / 2.0
    c = EARQ * MINBW
    d = math.log(LOW_FREQ + c) - math.log(high + c)
    return np.array([-c + math.exp(i * d / CHANNELS) * (high + c) for i in range(1, CHANNELS + 1)])


def erb(cf):
    return cf / EARQ + MINBW


def gammatone_sections(fs):
    """(b [23, 4, 3], a [23, 3], gain [23]): the four numerators of each channel in running order
    (the first already divided by `gain`), the common denominator and the magnitude of the
    unnormalised cascade at the centre frequency."""
    cfs = centre_freqs(fs)
    T = 1.0 / fs
    b = np.zeros((CHANNELS, 4, 3))
    a = np.zeros((CHANNELS, 3))
    gain = np.zeros(CHANNELS)
    r1, r2 = math.sqrt(3.0 + 2.0 ** 1.5), math.sqrt(3.0 - 2.0 ** 1.5)
    for i, cf in enumerate(cfs):
        B = 1.019 * 2.0 * math.pi * erb(cf)
        c, s, g = math.cos(2.0 * math.pi * cf * T), math.sin(2.0 * math.pi * cf * T), math.exp(-B * T)
        a[i] = (1.0, -2.0 * c * g, g * g)
        for j, (sign, r) in enumerate(((1.0, r1), (-1.0, r1), (1.0, r2), (-1.0, r2))):
            b[i, j] = (T, -(2.0 * T * c * g + sign * 2.0 * r * T * s * g) / 2.0, 0.0)
        zi = np.exp(-2j * math.pi * cf * T)       # z^-1 at the centre frequency
        den = a[i, 0] + a[i, 1] * zi + a[i, 2] * zi * zi
        h = 1.0 + 0.0j
        for j in range(4):
            h = h * ((b[i, j, 0] + b[i, j, 1] * zi) / den)
        gain[i] = abs(h)
        b[i, 0] /= gain[i]
    return b, a, gain


def slaney_gain(fs):
    """Slaney's closed form of the same gains (MakeERBFilters)."""
    cfs = centre_freqs(fs)
    T = 1.0 / fs
    B = 1.019 * 2.0 * np.pi * erb(cfs)
    e = np.exp(4j * cfs * np.pi * T)
    k1 = 2.0 * T * np.exp(-B * T + 2j * cfs * np.pi * T)
    co, si = np.cos(2 * cfs * np.pi * T), np.sin(2 * cfs * np.pi * T)
    rp, rm = np.sqrt(3 + 2 ** 1.5), np.sqrt(3 - 2 ** 1.5)
    num = ((-2 * e * T + k1 * (co - rm * si)) * (-2 * e * T + k1 * (co + rm * si)) *
           (-2 * e * T + k1 * (co - rp * si)) * (-2 * e * T + k1 * (co + rp * si)))
    den = (-2 / np.exp(2 * B * T) - 2 * e + 2 * (1 + e) / np.exp(B * T)) ** 4
    return np.abs(num / den)


def modulation_centres():
    return np.array([4.0 * math.pow(32.0, k / 7.0) for k in range(BANDS)])


def modulation_sections(fs):
    """(b [8, 3], a [8, 3], left cutoffs c_k [8]) of the Q = 2 band-passes, a unnormalised."""
    f = modulation_centres()
    W = np.array([math.tan(math.pi * fk / fs) for fk in f])
    B0 = W / 2.0
    b = np.stack([B0, np.zeros(BANDS), -B0], axis=1)
    a = np.stack([1.0 + B0 + W * W, 2.0 * W * W - 2.0, 1.0 - B0 + W * W], axis=1)
    return b, a, f - B0 * fs / (2.0 * np.pi)


def frame_sizes(fs):
    return int(math.ceil(0.256 * fs)), int(math.ceil(0.064 * fs))


def n_frames(N, fs):
    wl, wi = frame_sizes(fs)
    return 0 if N < wl else 1 + (N - wl) // wi


def hamming_periodic(wl, dtype=np.float64):
    w = [0.54 - 0.46 * math.cos(2.0 * math.pi * n / wl) for n in range(wl)]
    return np.array(w).astype(dtype)


def gammatone(x, fs, dtype=np.float64):
    """y [23, N]: the channels of x."""
    b, a, _ = gammatone_sections(fs)
    x = np.asarray(x).astype(dtype)
    y = np.empty((CHANNELS, len(x)), dtype)
    for i in range(CHANNELS):
        v = x
        for j in range(4):
            v = lfilter(b[i, j].astype(dtype), a[i].astype(dtype), v)
        y[i] = v
    return y


def envelope(y, exact=False):
    """|analytic(y)| of each row of y [.., N] (fp64 transforms)."""
    y = np.asarray(y, dtype=np.float64)
    N = y.shape[-1]
    L = N if exact else 1 << max(N - 1, 0).bit_length()
    Y = np.fft.fft(y, L, axis=-1)
    h = np.zeros(L)
    if L % 2 == 0:
        h[0] = h[L // 2] = 1.0
        h[1:L // 2] = 2.0
    else:
        h[0] = 1.0
        h[1:(L + 1) // 2] = 2.0
    return np.abs(np.fft.ifft(Y * h, axis=-1)[..., :N])


def kstar_of(bw, cutoffs):
    if bw > cutoffs[7]:
        return 8
    if cutoffs[6] < bw < cutoffs[7]:
        return 7
    if cutoffs[5] < bw < cutoffs[6]:
        return 6
    return 5          # c_4 < BW < c_5, and BW <= c_4 or on a cutoff, which the toolbox leaves open


def stages(x, fs=16000, dtype=np.float64, exact=False):
    """Every stage of the measure for one row: a dict with 'cfs' [23], 'envelope_energy' [23]
    (sum of e_i^2 over the N samples), 'energy' [23, 8] (Ebar), 'share' (the cumulated share that
    decided BW, per cent), 'bw', 'kstar', 'srmr'."""
    if fs not in RATES:
        raise ValueError('srmr: rate must be 8000 or 16000, got {}'.format(fs))
    x = np.asarray(x)
    if x.ndim != 1:
        raise ValueError('srmr: one row, got shape {}'.format(x.shape))
    N = len(x)
    cfs = centre_freqs(fs)
    wl, wi = frame_sizes(fs)
    nf = n_frames(N, fs)
    nan = dict(cfs=cfs, envelope_energy=np.zeros(CHANNELS), energy=np.zeros((CHANNELS, BANDS)),
               share=float('nan'), bw=float('nan'), kstar=0, srmr=float('nan'))
    if nf == 0:
        return nan
    env = envelope(gammatone(x, fs, dtype).astype(np.float64), exact)
    mb, ma, cutoffs = modulation_sections(fs)
    w = hamming_periodic(wl, dtype)
    energy = np.zeros((CHANNELS, BANDS), dtype)
    e = env.astype(dtype)
    for k in range(BANDS):
        m = lfilter(mb[k].astype(dtype), ma[k].astype(dtype), e, axis=-1)
        acc = np.zeros(CHANNELS, dtype)
        for f in range(nf):
            seg = m[:, f * wi:f * wi + wl] * w
            acc += np.sum(seg * seg, axis=-1)
        energy[:, k] = acc / nf
    env_energy = np.sum(e * e, axis=-1)
    total = np.sum(energy)
    out = dict(cfs=cfs, envelope_energy=env_energy.astype(np.float64),
               energy=energy.astype(np.float64), share=float('nan'), bw=float('nan'), kstar=0,
               srmr=float('nan'))
    if not total > 0:
        return out
    per_channel = np.sum(energy, axis=1)
    cum = dtype(0)
    bw = float(erb(cfs[0]))
    share = float('nan')
    for i in range(CHANNELS - 1, -1, -1):      # from the lowest centre frequency upwards
        cum = cum + dtype(100) * per_channel[i] / total
        if cum > 90:
            bw, share = float(erb(cfs[i])), float(cum)
            break
    ks = kstar_of(bw, cutoffs)
    num = np.sum(energy[:, :4])
    den = np.sum(energy[:, 4:ks])
    out.update(share=share, bw=bw, kstar=ks, srmr=float(num / den))
    return out


def srmr(x, fs=16000, dtype=np.float64, exact=False):
    return stages(x, fs, dtype, exact)['srmr']
