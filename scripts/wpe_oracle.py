"""The numpy oracle of the WPE dereverberation baseline: the definition
that segan_dereverb.hip, ops.wpe_rows and baselines.wpe implement.

WPE, weighted prediction error or variance-normalised delayed linear prediction (Nakatani,
Yoshioka, Kinoshita, Miyoshi and Juang, IEEE TASLP 2010), in its single-channel STFT form, written
from the literature.  Per row of L samples at srate (16000 or 8000), with K = taps (1 .. 32),
D = delay (1 .. 8) and `iterations` (0 .. 8):

  1. N = 512, H = 128 at 16 kHz (N = 256, H = 64 at 8 kHz), F = N / 2 + 1 bins.  The window
     w[n] = sqrt(0.5 - 0.5 cos(2 pi n / N)) serves analysis and synthesis.  nf = ceil(L / H) + 3
     frames; frame j covers the samples (j - 3) H .. (j - 3) H + N - 1, samples outside [0, L) read
     as zero; Y[k][j] is the DFT of the windowed frame.
  2. A row with nf <= D + K, or with L = 0, is returned unchanged (a copy, bit for bit); its X is
     its Y and its g is zero.
  3. Per bin k, with X = Y and g = 0 at the start, `iterations` times:
       p_t = |X_t|^2 = re^2 + im^2, m = max_t p_t;           m = 0: g = 0, the bin stops
       lambda_t = max(p_t, 1e-10 m)
       y~_t = (Y_{t-D}, .., Y_{t-D-K+1})^T, zeros before the first frame
       R = sum_t y~_t y~_t^H (1 / lambda_t),  P = sum_t y~_t conj(Y_t) (1 / lambda_t)
       tr R = 0: g = 0, the bin stops
       R += 1e-10 (tr R / K) I
       g = R^-1 P by an unpivoted lower Cholesky R = L L^H and two substitutions; a pivot that is
       not positive gives g = 0, sets ST_PIVOT (bit 1, value 2) in the row's status, and the bin
       stops
       X_t = Y_t - g^H y~_t
  4. The inverse real DFT of each X[:, j] (the imaginary parts of the bins 0 and N / 2 ignored),
     times w, overlap-added in ascending j, times 1 / 2 (the four squared windows over a sample add
     up to 2); y[0 .. L).

Every floor and the diagonal loading are relative to the bin's own level, so a row times a power
of two gives the same bits times that power.  The order of the sums over t is NOT part of the
definition: the kernels add in ascending t, numpy adds pairwise, and the tolerances of the GPU
tests (100 times the oracle's own float64-to-longdouble movement, scripts/make_golden_wpe.py)
cover the difference.

The FFT, the Cholesky factorisation and the substitutions are written here, generic in dtype
(float64 or numpy.longdouble): numpy.fft and numpy.linalg do not do long double.

Known limitation: single-channel WPE assumes that the source is uncorrelated beyond the delay.  A
steady harmonic tone is predictable from its own past, so WPE cancels the source itself; it helps
on signals whose pitch and formants move, as speech's do.
"""
import numpy as np

RATES = (16000, 8000)
TAPS = (1, 32)
DELAY = (1, 8)
ITERATIONS = (0, 8)
FLOOR = 1e-10                # lambda_t >= FLOOR max_t p_t
LOADING = 1e-10              # R += LOADING (tr R / K) I
PAD_FRAMES = 3               # frames before the first sample's own
ST_PIVOT = 2                 # status bit 1: a bin's Cholesky met a pivot that is not positive


def constants(srate):
    """(N, H, F) at srate."""
    if isinstance(srate, bool) or srate not in RATES:
        raise ValueError('wpe: srate must be one of {}, got {!r}'.format(RATES, srate))
    N = 512 if srate == 16000 else 256
    return N, N // 4, N // 2 + 1


def n_frames(L, srate=16000):
    _, H, _ = constants(srate)
    return -(-L // H) + PAD_FRAMES


def _check(name, v, lo_hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo_hi[0] <= v <= lo_hi[1]:
        raise ValueError('wpe: {} must be an integer in {} .. {}, got {!r}'.format(
            name, lo_hi[0], lo_hi[1], v))


def _pi(dtype):
    return np.arctan(dtype(1)) * dtype(4)


def _ctype(dtype):
    return np.complex128 if dtype == np.float64 else np.clongdouble


def window(N, dtype=np.float64):
    n = np.arange(N).astype(dtype)
    return np.sqrt(dtype(0.5) - dtype(0.5) * np.cos(dtype(2) * _pi(dtype) * n / dtype(N)))


def fft(x, inverse=False, dtype=np.float64):
    """The DFT along the last axis (a power of two), unscaled in both directions: radix 2,
    decimation in time, in `dtype`'s complex type."""
    x = np.asarray(x).astype(_ctype(dtype))
    n = x.shape[-1]
    ang = dtype(2) * _pi(dtype) * np.arange(n // 2).astype(dtype) / dtype(n)
    tw = np.empty(n // 2, _ctype(dtype))
    tw.real = np.cos(ang)
    tw.imag = np.sin(ang) if inverse else -np.sin(ang)
    if n >= 4:
        tw[n // 4] = 1j if inverse else -1j

    def rec(v, t):
        m = v.shape[-1]
        if m == 1:
            return v
        e, o = rec(v[..., ::2], t[::2]), rec(v[..., 1::2], t[::2])
        o = o * t[:m // 2]
        return np.concatenate([e + o, e - o], axis=-1)

    return rec(x, tw)


def stft(x, srate=16000, dtype=np.float64):
    """Y [F, nf] of the row x."""
    N, H, F = constants(srate)
    x = np.asarray(x).astype(dtype)
    L = len(x)
    nf = n_frames(L, srate)
    xp = np.zeros((nf + 3) * H, dtype)
    xp[PAD_FRAMES * H:PAD_FRAMES * H + L] = x
    frames = xp[np.arange(nf)[:, None] * H + np.arange(N)[None, :]] * window(N, dtype)
    return np.ascontiguousarray(fft(frames, False, dtype)[:, :F].T)


def istft(X, L, srate=16000, dtype=np.float64):
    """y [L] of X [F, nf]."""
    N, H, F = constants(srate)
    nf = X.shape[1]
    Z = np.zeros((nf, N), _ctype(dtype))
    Z[:, :F] = X.T
    Z[:, 0] = X[0].real
    Z[:, N // 2] = X[F - 1].real
    Z[:, F:] = np.conj(X[1:F - 1][::-1].T)
    fr = (fft(Z, True, dtype).real * (dtype(1) / dtype(N))) * window(N, dtype)
    acc = np.zeros((nf + 3) * H, dtype)
    for j in range(nf):
        acc[j * H:j * H + N] += fr[j]
    return (acc * dtype(0.5))[PAD_FRAMES * H:PAD_FRAMES * H + L]


def _abs2(z):
    return z.real * z.real + z.imag * z.imag


def solve(R, P, dtype=np.float64):
    """g [B, K] with R g = P for the Hermitian R [B, K, K] (the lower triangle is read) by an
    unpivoted lower Cholesky, and ok [B]: False where a pivot was not positive (g is then 0)."""
    B, K = P.shape
    Lm = np.zeros((B, K, K), _ctype(dtype))
    diag = np.ones((B, K), dtype)
    ok = np.ones(B, bool)
    for j in range(K):
        d = R[:, j, j].real.copy()
        for k in range(j):
            d = d - _abs2(Lm[:, j, k])
        ok &= d > 0
        d = np.sqrt(np.where(ok, d, dtype(1)))
        diag[:, j] = d
        for i in range(j + 1, K):
            s = R[:, i, j].copy()
            for k in range(j):
                s = s - Lm[:, i, k] * np.conj(Lm[:, j, k])
            Lm[:, i, j] = s / d
    z = np.zeros((B, K), _ctype(dtype))
    rhs = P.copy()
    for k in range(K):                           # L z = P, column by column
        z[:, k] = rhs[:, k] / diag[:, k]
        for i in range(k + 1, K):
            rhs[:, i] = rhs[:, i] - Lm[:, i, k] * z[:, k]
    g = np.zeros((B, K), _ctype(dtype))
    rhs = z.copy()
    for k in range(K - 1, -1, -1):               # L^H g = z
        g[:, k] = rhs[:, k] / diag[:, k]
        for i in range(k):
            rhs[:, i] = rhs[:, i] - np.conj(Lm[:, k, i]) * g[:, k]
    g[~ok] = 0
    return g, ok


def filter_stft(Y, taps=10, delay=3, iterations=3, dtype=np.float64):
    """Step 3 on Y [F, nf] (nf > delay + taps): (X [F, nf], g [F, taps], status)."""
    ct = _ctype(dtype)
    Y = np.asarray(Y).astype(ct)
    F, nf = Y.shape
    K = taps
    pad = np.concatenate([np.zeros((F, delay + K - 1), ct), Y], axis=1)
    Yd = [pad[:, K - 1 - a:K - 1 - a + nf] for a in range(K)]     # Yd[a][:, t] = Y[:, t - D - a]
    X = Y.copy()
    g = np.zeros((F, K), ct)
    live = np.ones(F, bool)
    status = 0
    for _ in range(iterations):
        p = _abs2(X)
        m = p.max(axis=1)
        stop = live & ~(m > 0)
        run = live & (m > 0)
        inv = dtype(1) / np.maximum(p, dtype(FLOOR) * np.where(m > 0, m, dtype(1))[:, None])
        R = np.zeros((F, K, K), ct)
        P = np.zeros((F, K), ct)
        for a in range(K):
            for b in range(a + 1):
                R[:, a, b] = np.sum(Yd[a] * np.conj(Yd[b]) * inv, axis=1)
            P[:, a] = np.sum(Yd[a] * np.conj(Y) * inv, axis=1)
        tr = np.zeros(F, dtype)
        for a in range(K):
            tr = tr + R[:, a, a].real
        stop |= run & ~(tr > 0)
        run &= tr > 0
        load = dtype(LOADING) * (np.where(tr > 0, tr, dtype(1)) / dtype(K))
        for a in range(K):
            R[:, a, a] = R[:, a, a].real + load
        gn, ok = solve(R, P, dtype)
        bad = run & ~ok
        if bad.any():
            status |= ST_PIVOT
        stop |= bad
        run &= ok
        g[run] = gn[run]
        g[stop] = 0
        live = run
        pred = np.zeros((F, nf), ct)
        for a in range(K):
            pred = pred + np.conj(g[:, a])[:, None] * Yd[a]
        X = Y - pred
    return X, g, status


def wpe(x, srate=16000, taps=10, delay=3, iterations=3, dtype=np.float64):
    """One row x [L] -> dict: 'y' [L] (dtype), 'nframes', 'status', 'Y' and 'X' [F, nf], 'g'
    [F, taps] (complex)."""
    N, H, F = constants(srate)
    _check('taps', taps, TAPS)
    _check('delay', delay, DELAY)
    _check('iterations', iterations, ITERATIONS)
    x = np.asarray(x).astype(dtype)
    L = len(x)
    nf = n_frames(L, srate)
    Y = stft(x, srate, dtype)
    if L == 0 or nf <= delay + taps:
        return {'y': x.copy(), 'nframes': nf, 'status': 0, 'Y': Y, 'X': Y.copy(),
                'g': np.zeros((F, taps), _ctype(dtype))}
    X, g, status = filter_stft(Y, taps, delay, iterations, dtype)
    return {'y': istft(X, L, srate, dtype), 'nframes': nf, 'status': status, 'Y': Y, 'X': X, 'g': g}
