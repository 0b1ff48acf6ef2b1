"""fp64 numpy oracle of the noise-excited LPC resynthesis ("whisper") of `ops.whisper_rows` (DESIGN.md
section 18).  Every default is this project's own choice.

    philox4x32_10(ctr, key)                       -> the four output words (uint32 arrays)
    noise(seed, j0, count, dtype)                 -> u[j0 .. j0 + count - 1]
    hann(dtype), lag_window(lag_hz, dtype)        -> the two tables
    lags(x, length, prev, lag_hz, dtype)          -> r [F, P + 1]
    lpc(r, dtype)                                 -> (a [F, P + 1], sigma [F], order [F])
    whisper(x, seed, tilt, length=None, prev=0.0, lag_hz=120.0, dtype=np.float64)
        -> dict(r, a, sigma, order, y (y[0 .. len] after the peak guard), peak, status, nsilent,
                minorder, out [T], prev_out)
    voiced(f0, T, seed)                           -> the periodic test row of the fixture and tests

dtype is np.float64 (the kernels' arithmetic, operation for operation) or np.longdouble (the same
operations in the platform's widest format: how far rounding moves the fp64 result).  The two
tables are rounded to fp64 in either mode: they are inputs, the kernels get these very numbers.
"""
import numpy as np

N = 512            # frame
H = 256            # hop
P = 16             # order
WU = 256           # warm-up samples of the synthesis filter
SRATE = 16000
WHITE = 1.0001     # r[0] is multiplied by this
EFLOOR = 2.0 ** -40
WSUM2 = 192.0      # sum of w^2 of the periodic Hann window of 512
J0 = 1 << 20       # counter of sample j is j + J0
C = float.fromhex('0x1.279a74590331cp+31')   # sqrt((2^64 - 1) / 3)
WHISPER_SILENT = 1
WHISPER_TILT = 2

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11; Random123).  ctr: four, key: two arrays (or
    scalars) of 32-bit words held in uint64."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in ctr]
    k = [np.asarray(v, dtype=np.uint64) & _MASK for v in key]
    s32 = np.uint64(32)
    for rnd in range(10):
        if rnd:
            k = [(k[0] + np.uint64(_W0)) & _MASK, (k[1] + np.uint64(_W1)) & _MASK]
        p0 = np.uint64(_M0) * c[0]
        p1 = np.uint64(_M1) * c[2]
        c = [((p1 >> s32) ^ c[1] ^ k[0]) & _MASK, p1 & _MASK,
             ((p0 >> s32) ^ c[3] ^ k[1]) & _MASK, p0 & _MASK]
    return c


def _check_vectors():
    ones = 0xFFFFFFFF
    for ctr, key, want in (
            ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((ones,) * 4, (ones,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
             (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = tuple(int(v) for v in philox4x32_10(ctr, key))
        assert got == want, 'Philox4x32-10 misses a Random123 vector: {} != {}'.format(got, want)


_check_vectors()
assert C == np.sqrt(np.float64((2 ** 64 - 1) / 3))


def noise(seed, j0, count, dtype=np.float64):
    """u[j], j = j0 .. j0 + count - 1: zero mean, unit variance; the sum of four words is integer
    arithmetic, the division one operation."""
    seed = int(seed) & ((1 << 64) - 1)
    J = np.array([(int(j0) + i + J0) & ((1 << 64) - 1) for i in range(int(count))], dtype=np.uint64)
    w = philox4x32_10((J & _MASK, J >> np.uint64(32), 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    s = (w[0] + w[1] + w[2] + w[3]).astype(np.int64) - np.int64(2 * (2 ** 32 - 1))
    return s.astype(dtype) / dtype(C)


def hann(dtype=np.float64):
    m = np.arange(N, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * m / N)).astype(dtype)


def lag_window(lag_hz=120.0, dtype=np.float64):
    lag = np.arange(P + 1, dtype=np.float64)
    return np.exp(-0.5 * (2.0 * np.pi * float(lag_hz) * lag / SRATE) ** 2).astype(dtype)


def _length(x, length):
    T = len(x)
    return T if length is None else min(max(int(length), 0), T)


def nframes(length):
    return length // H + 2


def _extended(x, n, prev, dtype):
    """xe[j] for j = -H .. (F + 1) H - 1 (offset H), zero outside 0 .. n"""
    F = nframes(n)
    xe = np.zeros((F + 2) * H, dtype=dtype)
    xe[H] = dtype(np.float32(prev))
    xe[H + 1:H + 1 + n] = x[:n].astype(dtype)
    return xe


def lags(x, length=None, prev=0.0, lag_hz=120.0, dtype=np.float64):
    """r [F, P + 1].  Per frame, s = w xe; lane i of 64 sums s[m] s[m + l] over m = i, i + 64, ..
    ascending (terms past the frame are zero), the 64 partial sums are added by the butterfly v[i] +
    v[i ^ o], o = 32, 16 .. 1; then the lag window and the factor on r[0]."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = _length(x, length)
    F = nframes(n)
    xe = _extended(x, n, prev, dtype)
    w = hann(dtype)
    g = lag_window(lag_hz, dtype)
    r = np.zeros((F, P + 1), dtype=dtype)
    for f in range(F):
        s = np.zeros(N + P, dtype=dtype)
        s[:N] = w * xe[f * H:f * H + N]           # frame f starts at j = (f - 1) H
        for l in range(P + 1):
            prod = (s[:N] * s[l:l + N]).reshape(N // 64, 64)
            v = np.zeros(64, dtype=dtype)
            for i in range(N // 64):
                v = v + prod[i]
            for o in (32, 16, 8, 4, 2, 1):
                v = v[:o] + v[o:2 * o]
            r[f, l] = v[0] * g[l]
        r[f, 0] = r[f, 0] * dtype(WHITE)
    return r


def lpc(r, dtype=np.float64):
    """Levinson-Durbin on each row of r [F, P + 1], in the operation order of the kernels'
    `levinson_lpc`: (a [F, P + 1] with a[0] = 1, sigma, order).  A row with r[0] <= 0 (or NaN) is
    silent: a = [1, 0 ..], sigma = 0, order = 0."""
    r = np.asarray(r, dtype=dtype).reshape(-1, P + 1)
    F = r.shape[0]
    A = np.zeros((F, P + 1), dtype=dtype)
    A[:, 0] = 1
    sigma = np.zeros(F, dtype=dtype)
    order = np.zeros(F, dtype=np.int32)
    for f in range(F):
        R = r[f]
        if not R[0] > 0:
            continue
        a = np.zeros(P, dtype=dtype)
        E = R[0]
        floor = dtype(EFLOOR) * R[0]
        m = 0
        for i in range(P):
            if not E > floor:
                break
            s = dtype(0)
            for j in range(i):
                s = s + a[j] * R[i - j]
            rc = (R[i + 1] - s) / E
            if not abs(rc) < 1:
                break
            na = a.copy()
            for j in range(i):
                na[j] = a[j] - rc * a[i - 1 - j]
            na[i] = rc
            a = na
            E = (1 - rc * rc) * E
            m = i + 1
        A[f, 1:m + 1] = -a[:m]
        sigma[f] = np.sqrt(E / dtype(WSUM2))
        order[f] = m
    return A, sigma, order


def whisper(x, seed, tilt, length=None, prev=0.0, lag_hz=120.0, dtype=np.float64):
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    T = len(x)
    n = _length(x, length)
    F = nframes(n)
    prev32 = np.float32(prev)
    r = lags(x, n, prev32, lag_hz, dtype)
    a, sigma, order = lpc(r, dtype)
    silent = ~(r[:, 0] > 0)
    nsilent = int(silent.sum())
    minorder = int(order[~silent].min()) if nsilent < F else P
    tilt = float(tilt)
    status = (0 if 0.0 <= tilt < 1.0 else WHISPER_TILT) | (WHISPER_SILENT if nsilent == F else 0)
    res = dict(r=r, a=a, sigma=sigma, order=order, status=status, nsilent=nsilent,
               minorder=minorder)
    if status:
        res.update(y=np.concatenate([[prev32], x[:n]]).astype(dtype), peak=dtype(0), out=x.copy(),
                   prev_out=prev32)
        return res

    # the excitation of all frames at once: frame f runs j = (f - 1) H - WU .. (f + 1) H - 1
    steps = WU + N
    u = noise(seed, -H - WU - 1, (F - 1) * H + steps + 1, dtype)     # u[j], offset H + WU + 1
    tau = dtype(tilt)
    den = np.sqrt(1 + tau * tau)
    v = np.zeros((F, steps + P), dtype=dtype)                        # P zeros of state in front
    w = hann(dtype)
    base = np.arange(F) * H                                          # index of u[j - 1] at step 0
    for t in range(steps):
        e = (sigma * (u[base + t + 1] - tau * u[base + t])) / den
        acc = e
        for k in range(P, 0, -1):
            acc = acc - a[:, k] * v[:, P + t - k]
        v[:, P + t] = acc
    wv = w[None, :] * v[:, P + WU:]
    wv[silent] = 0
    y = np.zeros(n + 1, dtype=dtype)
    j = np.arange(n + 1)
    q = j // H
    y = wv[q, j - q * H + H] + wv[q + 1, j - q * H]                  # the earlier frame first
    peak = np.abs(y).max()
    if peak > 1:
        y = y / peak
    out = np.zeros(T, dtype=dtype)
    out[:n] = y[1:]
    res.update(y=y, peak=peak, out=out, prev_out=y[0])
    return res


def voiced(f0, T, seed, peak=0.5):
    """A periodic test row: an impulse train at f0 plus 1 % white noise through three two-pole
    resonances (700 / 1200 / 2600 Hz, bandwidths 80 / 100 / 150 Hz) in cascade, under a slow
    Hann-shaped envelope, scaled to `peak` and quantised to int16 steps; float32."""
    rng = np.random.RandomState(seed)
    period = SRATE / float(f0)
    e = 0.01 * rng.standard_normal(T)
    k = 0
    while int(round(k * period)) < T:
        e[int(round(k * period))] += 1.0
        k += 1
    y = e
    for fc, bw in ((700.0, 80.0), (1200.0, 100.0), (2600.0, 150.0)):
        rad = np.exp(-np.pi * bw / SRATE)
        b1, b2 = 2.0 * rad * np.cos(2.0 * np.pi * fc / SRATE), -rad * rad
        z = np.zeros(T)
        z1 = z2 = 0.0
        for i in range(T):
            z0 = y[i] + b1 * z1 + b2 * z2
            z[i] = z0
            z2, z1 = z1, z0
        y = z
    env = 0.55 - 0.45 * np.cos(2.0 * np.pi * np.arange(T) / T)
    y = y * env
    y = y * (peak / np.abs(y).max())
    return (np.round(y * 32768.0) / 32768.0).astype(np.float32)
