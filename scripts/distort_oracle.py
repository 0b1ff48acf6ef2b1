"""fp64 numpy oracle of the three signal-level distortions: amplitude
clipping, chunk removal and zero-phase band limiting, as `ops.clip_rows`, `ops.chop_rows` and
`ops.fir_rows` define them.

    clip(x, factor, length=None, prev=None) -> dict(y, prev, m, thr, nclipped, status)
    chop(x, q, c0, u, dur, length=None)     -> dict(y, starts, nactive, nzeroed, status)
    fir(x, h, length=None, prev=None)       -> (y fp64, y[-1])   the kernel's order of operations
    fir_convolve(x, h, length=None, prev=None) -> the same by np.convolve of the two-sided filter
    lowpass(fc, srate, zeros, beta)         -> (K, one-sided taps h[0 .. K])

The clip works on fp32 values (a max and two comparisons are exact; the threshold is one fp64
product rounded to fp32), the chop on integers; only the FIR rounds, and `fir` rounds exactly where
the kernel does: the inner sum xe[n-k] + xe[n+k], its product with h[k] and the accumulation, k
ascending, all in float64.
"""
import numpy as np

CLIP_SILENT = 1
CLIP_FACTOR = 2
CHOP_NOLEVEL = 1
CHOP_MAX = 8
FIR_MAX_K = 2048


def _length(x, length):
    T = len(x)
    return T if length is None else min(max(int(length), 0), T)


def clip(x, factor, length=None, prev=None):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = _length(x, length)
    m = np.float32(np.abs(x[:n]).max()) if n else np.float32(0)
    status = (CLIP_SILENT if n == 0 or m == 0 else 0) | \
        (0 if 0.0 < float(factor) <= 1.0 else CLIP_FACTOR)
    thr = np.float32(0) if status & CLIP_FACTOR else np.float32(np.float64(factor) * np.float64(m))
    y = x.copy()
    p = None if prev is None else np.float32(prev)
    if not status:
        y[:n] = np.minimum(np.maximum(x[:n], -thr), thr)
        if p is not None:
            p = np.float32(min(max(p, -thr), thr))
    return dict(y=y, prev=p, m=m, thr=thr, nclipped=int(np.count_nonzero(y != x)), status=status)


def chop(x, q, c0, u, dur, length=None):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    dur = np.asarray(dur, dtype=np.int64).reshape(-1)
    assert len(q) == len(x) and len(u) == len(dur) <= CHOP_MAX
    L = _length(x, length)
    c0 = np.nan if c0 is None else float(c0)
    active = np.nonzero(q[:L] >= c0)[0] if not np.isnan(c0) else np.zeros(0, dtype=np.int64)
    n = len(active)
    starts = np.full(len(u), -1, dtype=np.int64)
    y = x.copy()
    if n == 0:
        return dict(y=y, starts=starts, nactive=0, nzeroed=0, status=CHOP_NOLEVEL)
    mask = np.zeros(len(x), dtype=bool)
    for c in range(len(u)):
        if dur[c] <= 0:
            continue
        k = min(int(np.floor(u[c] * np.float64(n))), n - 1)
        starts[c] = active[k]
        mask[starts[c]:min(starts[c] + dur[c], L)] = True
    y[mask] = 0
    return dict(y=y, starts=starts, nactive=n, nzeroed=int(mask.sum()), status=0)


def _extended(x, K, length, prev):
    """xe[n], n = -1 - K .. T - 1 + K, as float64: prev at -1, x on 0 .. len-1, zero elsewhere."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    T, L = len(x), _length(x, length)
    xe = np.zeros(T + 1 + 2 * K)
    xe[K] = 0.0 if prev is None else np.float64(prev)
    xe[K + 1:K + 1 + L] = x[:L]
    return xe, T, L


def fir(x, h, length=None, prev=None):
    """y[n] = h[0] xe[n] + sum_{k=1..K} h[k] (xe[n-k] + xe[n+k]), n = -1 .. len-1, in the kernel's
    order; zero from len on.  Returns (y [T] float64, y[-1])."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    K = len(h) - 1
    xe, T, L = _extended(x, K, length, prev)
    acc = h[0] * xe[K:K + T + 1]
    for k in range(1, K + 1):
        acc = acc + h[k] * (xe[K - k:K - k + T + 1] + xe[K + k:K + k + T + 1])
    y = acc[1:].copy()
    y[L:] = 0.0
    return y, acc[0]


def fir_convolve(x, h, length=None, prev=None):
    """The same filter as np.convolve of the two-sided taps (another order of summation)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    K = len(h) - 1
    xe, T, L = _extended(x, K, length, prev)
    full = np.convolve(xe, np.concatenate((h[:0:-1], h)))      # index i <-> n = i - 1 - 2K
    acc = full[2 * K:2 * K + T + 1]
    y = acc[1:].copy()
    y[L:] = 0.0
    return y, acc[0]


def fir_bound(h, xmax):
    """2 (K + 1) 2^-53 sum_{k=0..K} |h[k]| max|x|: the bound between two orders of the sum."""
    h = np.asarray(h, dtype=np.float64)
    return 2 * len(h) * 2.0 ** -53 * float(np.abs(h).sum()) * float(xmax)


def lowpass(fc, srate=16000, zeros=32, beta=8.6):
    """(K, h[0 .. K]) of the Kaiser-windowed sinc low-pass with cutoff fc: K = ceil(zeros srate /
    (2 fc)), h[k] = sinc(2 fc k / srate) w(k), scaled to unit DC gain.  Restates
    augment.lowpass_bank's arithmetic: keep the two alike."""
    K = int(np.ceil(zeros * srate / (2.0 * fc)))
    k = np.arange(K + 1, dtype=np.float64)
    if K == 0:
        return 0, np.ones(1)
    w = np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - (k / K) ** 2))) / np.i0(beta)
    h = np.sinc(2.0 * fc * k / srate) * w
    return K, h / (h[0] + 2.0 * h[1:].sum())
