"""fp64 numpy / scipy oracle of STOI, Taal et al.'s short-time objective intelligibility
(DESIGN.md section 10 states the rules it follows).  It checks the HIP kernels behind ops.stoi:
scripts/make_golden_stoi.py runs it to write tests/golden/stoi.pt, and tests/test_stoi.py runs it
again against that fixture.  Needs numpy, scipy and resample_oracle.py next to it: the
resampling to 10 kHz is that oracle's, with scipy's default filter (10, 5.0).

    import stoi_oracle as S
    d = S.stoi(clean, processed, 16000)          # float, NaN where STOI is undefined
    st = S.stoi_stages(clean, processed, 16000)   # every intermediate as a dict
"""
import math

import numpy as np

from resample_oracle import design, ratio, resample, out_len as resampled_length  # noqa: F401

FS = 10000          # internal rate
N = 256             # frame
K = 128             # hop
NFFT = 512
J = 15              # third-octave bands
MN = 150.0          # centre of the lowest band, Hz
SEG = 30            # segment length in band frames
BETA = -15.0        # lower signal-to-distortion bound, dB
DYN = 40.0          # dynamic range of the silent-frame removal, dB
CLIP = 10.0 ** (-BETA / 20.0)
SRATE_MIN, SRATE_MAX = 4000, 48000


def window():
    """Hann window without zero end points: 0.5 * (1 - cos(2 pi (n+1) / (N+1))), n = 0..N-1."""
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(1, N + 1) / (N + 1)))


def band_edges():
    """[J, 2] int: the DFT bins [lo, hi) each third-octave band sums; the nearest bin (first of
    equals) to 150 * 2^((2i -+ 1)/6) Hz on the grid k * FS / NFFT, k = 0..NFFT/2."""
    f = np.arange(NFFT // 2 + 1) * FS / NFFT
    i = np.arange(J)
    lo = MN * 2.0 ** ((2 * i - 1) / 6.0)
    hi = MN * 2.0 ** ((2 * i + 1) / 6.0)
    return np.array([[np.argmin((f - a) ** 2), np.argmin((f - b) ** 2)] for a, b in zip(lo, hi)],
                    dtype=np.int64)


def plan(srate):
    """(p, q, taps) of the resampling srate -> FS: p / q = FS / srate in lowest terms and
    resample_oracle.design(p, q, 10, 5.0).  FS itself needs no resampling: (1, 1, [1.0])."""
    srate = int(srate)
    if not SRATE_MIN <= srate <= SRATE_MAX:
        raise ValueError('srate {} outside {} .. {} Hz'.format(srate, SRATE_MIN, SRATE_MAX))
    p, q = ratio(srate, FS)
    return p, q, design(p, q, 10, 5.0)


def resample_upfirdn(x, p, q, taps):
    """The same resampling the classic way: prepend zeros to the filter so that its centre
    falls on a multiple of q, append zeros until the output is long enough, upsample-filter-
    downsample with scipy.signal.upfirdn, drop the filter delay, keep ceil(Lx p / q) samples."""
    from scipy.signal import upfirdn
    x = np.asarray(x, dtype=np.float64)
    Lx = len(x)
    Ly = resampled_length(Lx, p, q)
    half = (len(taps) - 1) // 2
    pre = q - half % q
    delay = (half + pre) // q
    post = 0
    while resampled_length((Lx - 1) * p + len(taps) + pre + post, 1, q) < Ly + delay:
        post += 1
    h = np.concatenate([np.zeros(pre), taps, np.zeros(post)])
    return upfirdn(h, x, p, q)[delay:delay + Ly]


def n_frames(L):
    """Frames of N samples at hop K starting at 0, K, ... with the last start at most L - N - 1
    (a frame ending exactly at L is not taken)."""
    return (L - N - 1) // K + 1 if L > N else 0


def _frames(x, F):
    return x[np.arange(F)[:, None] * K + np.arange(N)]


def remove_silent_frames(x, y):
    """Frame energies of the clean x, the keep mask (within DYN dB of the loudest frame), and
    both signals' kept frames overlap-added windowed in order."""
    w = window()
    F = n_frames(len(x))
    with np.errstate(divide='ignore', invalid='ignore'):
        E = 20.0 * np.log10(np.linalg.norm(_frames(x, F) * w, axis=1) / np.sqrt(N))
        keep = (E - np.max(E) + DYN) > 0 if F else np.zeros(0, dtype=bool)
    kept = np.nonzero(keep)[0]
    M = len(kept)
    Lc = (M - 1) * K + N if M else 0
    xs, ys = np.zeros(Lc), np.zeros(Lc)
    for c, j in enumerate(kept):
        xs[c * K:c * K + N] += x[j * K:j * K + N] * w
        ys[c * K:c * K + N] += y[j * K:j * K + N] * w
    return E, keep, M, xs, ys


def band_envelopes(x):
    """[J, F'] third-octave band magnitudes of the frames of x, windowed again, 512-point DFT."""
    w = window()
    F = n_frames(len(x))
    spec = np.abs(np.fft.rfft(_frames(x, F) * w, NFFT, axis=1)) ** 2
    env = np.zeros((J, F))
    for i, (lo, hi) in enumerate(band_edges()):
        env[i] = np.sqrt(spec[:, lo:hi].sum(axis=1))
    return env


def segment_correlations(X, Y):
    """[S, J] correlation of each 30-frame segment m = 29 .. F'-1 of each band: the processed
    envelope scaled to the clean one's energy, clipped to X + X*CLIP with a NaN-ignoring minimum
    (np.fmin: an all-zero processed window gives alpha = inf, 0 * inf = NaN, and so X + X*CLIP),
    Pearson correlation (0/0 -> NaN)."""
    F = X.shape[1]
    S = max(F - SEG + 1, 0)
    rho = np.zeros((S, J))
    with np.errstate(divide='ignore', invalid='ignore'):
        for s in range(S):
            Xs, Ys = X[:, s:s + SEG], Y[:, s:s + SEG]
            alpha = np.sqrt(np.sum(Xs * Xs, axis=1) / np.sum(Ys * Ys, axis=1))
            Yp = np.fmin(alpha[:, None] * Ys, Xs + Xs * CLIP)
            xn = Xs - np.mean(Xs, axis=1, keepdims=True)
            xn = xn / np.sqrt(np.sum(xn * xn, axis=1, keepdims=True))
            yn = Yp - np.mean(Yp, axis=1, keepdims=True)
            yn = yn / np.sqrt(np.sum(yn * yn, axis=1, keepdims=True))
            rho[s] = np.sum(xn * yn, axis=1)
    return rho


def stoi_stages(x, y, srate):
    """Every intermediate of STOI of the clean x and processed y (1-D, equal lengths)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if x.shape != y.shape:
        raise ValueError('x and y have {} and {} samples'.format(len(x), len(y)))
    p, q, taps = plan(srate)
    xr, yr = (resample(x, p, q, taps), resample(y, p, q, taps)) if srate != FS else (x, y)
    E, keep, M, xs, ys = remove_silent_frames(xr, yr)
    X, Y = band_envelopes(xs), band_envelopes(ys)
    rho = segment_correlations(X, Y)
    d = float(np.mean(rho)) if M and rho.size else math.nan
    return dict(xr=xr, yr=yr, energy=E, mask=keep, M=M, xs=xs, ys=ys, X=X, Y=Y, rho=rho, d=d)


def stoi(x, y, srate):
    """STOI of the clean x and the processed y: float in (-1, 1], NaN when the clean signal has
    no frame above -inf dB, when fewer than 30 band frames remain, or when a segment's
    correlation is 0/0."""
    return stoi_stages(x, y, srate)['d']
