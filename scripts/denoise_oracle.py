"""The numpy oracle of the Wiener / log-MMSE baseline enhancers: the
definition that segan_denoise.hip, ops.denoise_rows and baselines.wiener / logmmse implement.

One short-time spectral enhancer with two gain rules on the decision-directed a-priori SNR of
Ephraim & Malah (1984) and the VAD-gated noise tracking of Loizou's `wiener_as` / `logmmse`
programs, written from the literature:

  wiener    G = xi / (1 + xi)                                         (Scalart & Filho 1996)
  logmmse   G = xi / (1 + xi) exp(E1(v) / 2), v = gamma xi / (1 + xi)  (Ephraim & Malah 1985)

Per row of L samples at srate (16000 or 8000): F = srate / 50 (20 ms), H = F / 2, N = 2 F.

  1. w[n] = 0.54 - 0.46 cos(2 pi n / (F - 1)), scaled by H / sum(w).
  2. m[k] = (|X_0[k]| + .. + |X_5[k]|) / 6 with X_j = DFT_N(w x[j F : (j + 1) F]), the six leading
     non-overlapping frames added in ascending j; lambda[k] = max(m[k]^2, 2^-100), k = 0 .. F.
  3. Frame t = 0 .. nf - 1, nf = L // H - 1: S = DFT_N(w x[t H : t H + F]), s2 = |S|^2 = re^2 +
     im^2, gamma = min(s2 / lambda, 40), xi = max(a P / lambda + (1 - a) max(gamma - 1, 0),
     10^-2.5) with a = 0.98 and P = |G S|^2 of the frame before (t = 0: the first term is a).
  4. l[k] = gamma xi / (1 + xi) - log(1 + xi); v_t = (sum_k c_k l[k]) / F with c_0 = c_F = 1, the
     others 2.  THE ORDER OF THIS SUM IS PART OF THE DEFINITION: bins are taken in groups of 64
     (k = 64 g .. 64 g + 63), each group added in ascending k from zero, then the group sums added
     in ascending g from zero: what a workgroup of waves of 64 lanes does with one lane per bin.
     v_t < 0.15: lambda <- max(0.98 lambda + 0.02 s2, 2^-100), after gamma and xi of this frame
     were formed and before nothing else: gain and P use gamma and xi as they are.
  5. A = xi / (1 + xi); G = A (wiener) or A exp(E1(max(A gamma, 2^-40)) / 2) (logmmse, unclipped);
     P <- (G G) s2.
  6. o_t = the first F samples of real(IDFT_N(G S)) with the Hermitian extension:
     o_t[n] = (sum_k c_k (re_k cos(2 pi k n / N) - im_k sin(2 pi k n / N))) / N;
     y[n] = sum_t o_t[n - t H], the earlier frame added first; y[n] = 0 for n >= (nf + 1) H.
  7. L < 6 F: the row is returned unchanged, nframes = 0.

Every DFT is a matrix product with a table of N twiddles indexed by (k n) mod N, so the whole
oracle runs unchanged in numpy.longdouble (`dtype=`): the movement between the two runs is what the
tolerances of the GPU tests are made of (scripts/make_golden_denoise.py).

E1, the exponential integral, is written here, generic in dtype: below 1 the power series
-gamma_E - ln x - sum_n (-x)^n / (n n!), from 1 on the modified Lentz continued fraction, both
stopped at a relative step of 2^-53 whatever the dtype.
"""
import numpy as np

RATES = (16000, 8000)
ALPHA = 0.98
ETA = 0.15                   # the VAD threshold on v_t
GAMMA_MAX = 40.0
XI_MIN = 10.0 ** -2.5
LAMBDA_MIN = 2.0 ** -100
E1_MIN = 2.0 ** -40
E1_STEP = 2.0 ** -53
E1_SERIES_MAX = 100          # terms of the series (x < 1 needs 18)
E1_LENTZ_MAX = 400           # steps of the continued fraction (x = 1 needs 92)
EULER = 0.5772156649015328606065120900824024
NOISE_FRAMES = 6
GROUP = 64
RULES = ('wiener', 'logmmse')


def constants(srate):
    """(F, H, N) at srate."""
    if isinstance(srate, bool) or srate not in RATES:
        raise ValueError('denoise: srate must be one of {}, got {!r}'.format(RATES, srate))
    F = srate // 50
    return F, F // 2, 2 * F


def n_frames(L, srate=16000):
    F, H, _ = constants(srate)
    return L // H - 1 if L >= NOISE_FRAMES * F else 0


def window(F, dtype=np.float64):
    n = np.arange(F).astype(dtype)
    w = dtype(0.54) - dtype(0.46) * np.cos(dtype(2) * _pi(dtype) * n / dtype(F - 1))
    return w * (dtype(F // 2) / np.cumsum(w)[-1])      # cumsum: the sum in ascending n


def _pi(dtype):
    return np.arctan(dtype(1)) * dtype(4)


def twiddles(N, dtype=np.float64):
    """(cos, sin)(2 pi m / N), m = 0 .. N - 1."""
    ang = dtype(2) * _pi(dtype) * np.arange(N).astype(dtype) / dtype(N)
    return np.cos(ang), np.sin(ang)


def dft_tables(F, dtype=np.float64):
    """C, S [F + 1, F]: cos and sin of 2 pi k n / N through the table, for the analysis; and
    Ci, Si [F, F + 1], the same for the synthesis with the Hermitian weights c_k folded in."""
    N = 2 * F
    c, s = twiddles(N, dtype)
    idx = (np.arange(F + 1)[:, None] * np.arange(F)[None, :]) % N
    C, S = c[idx], s[idx]
    ck = np.full(F + 1, 2.0).astype(dtype)
    ck[0] = ck[F] = 1
    return C, S, (C * ck[:, None]).T.copy(), (S * ck[:, None]).T.copy()


def exp1(x, dtype=np.float64):
    """E1(x) for x > 0, elementwise, in `dtype`; both branches stop at a relative step of 2^-53."""
    x = np.atleast_1d(np.asarray(x, dtype=dtype))
    out = np.zeros_like(x)
    step = dtype(E1_STEP)
    lo = x < 1
    if lo.any():
        z = x[lo]
        p = np.ones_like(z)
        acc = np.zeros_like(z)
        live = np.ones(z.shape, bool)
        for n in range(1, E1_SERIES_MAX + 1):
            p = p * (-z) / dtype(n)
            term = p / dtype(n)
            acc = np.where(live, acc + term, acc)
            live = live & ~(np.abs(term) <= step * np.abs(acc))
            if not live.any():
                break
        out[lo] = (-dtype(EULER) - np.log(z)) - acc
    hi = ~lo
    if hi.any():
        z = x[hi]
        b = z + dtype(1)
        c = np.full_like(z, np.finfo(np.float64).max)
        d = dtype(1) / b
        h = d.copy()
        live = np.ones(z.shape, bool)
        for i in range(1, E1_LENTZ_MAX + 1):
            a = -dtype(i) * dtype(i)
            b = b + dtype(2)
            d = dtype(1) / (a * d + b)
            c = b + a / c
            delta = c * d
            h = np.where(live, h * delta, h)
            live = live & ~(np.abs(delta - dtype(1)) <= step)
            if not live.any():
                break
        out[hi] = h * np.exp(-z)
    return out


def vad_sum(l, F, dtype=np.float64):
    """v_t of step 4 for l [F + 1]: groups of 64 bins, ascending inside, then ascending groups."""
    ng = (F + 1 + GROUP - 1) // GROUP
    t = np.zeros(ng * GROUP, dtype=dtype)
    t[:F + 1] = l * dtype(2)
    t[0], t[F] = l[0], l[F]
    t = t.reshape(ng, GROUP)
    acc = np.zeros(ng, dtype=dtype)
    for i in range(GROUP):
        acc = acc + t[:, i]
    v = dtype(0)
    for g in range(ng):
        v = v + acc[g]
    return v / dtype(F)


def denoise(x, srate=16000, rule='logmmse', dtype=np.float64):
    """One row x [L] -> dict: 'y' [L] (dtype), 'nframes', 'vad' [nf] (v_t), 'update' [nf] (bool:
    the noise estimate was updated at the frame), 'margin' [nf] (|v_t - 0.15|)."""
    if rule not in RULES:
        raise ValueError('denoise: rule must be one of {}, got {!r}'.format(RULES, rule))
    F, H, N = constants(srate)
    x = np.asarray(x).astype(dtype)
    L = len(x)
    nf = n_frames(L, srate)
    if nf == 0:
        return {'y': x.copy(), 'nframes': 0, 'vad': np.zeros(0, dtype), 'update': np.zeros(0, bool),
                'margin': np.zeros(0, np.float64)}
    w = window(F, dtype)
    C, S, Ci, Si = dft_tables(F, dtype)
    m = np.zeros(F + 1, dtype)
    for j in range(NOISE_FRAMES):
        seg = w * x[j * F:(j + 1) * F]
        re, im = C @ seg, -(S @ seg)
        m = m + np.sqrt(re * re + im * im)
    m = m / dtype(NOISE_FRAMES)
    lam = np.maximum(m * m, dtype(LAMBDA_MIN))
    a = dtype(ALPHA)
    b = dtype(1) - a
    y = np.zeros(L, dtype)
    vad = np.zeros(nf, dtype)
    upd = np.zeros(nf, bool)
    P = None
    for t in range(nf):
        seg = w * x[t * H:t * H + F]
        re, im = C @ seg, -(S @ seg)
        s2 = re * re + im * im
        gam = np.minimum(s2 / lam, dtype(GAMMA_MAX))
        first = np.full(F + 1, a) if P is None else a * P / lam
        xi = np.maximum(first + b * np.maximum(gam - dtype(1), dtype(0)), dtype(XI_MIN))
        l = gam * xi / (dtype(1) + xi) - np.log(dtype(1) + xi)
        v = vad_sum(l, F, dtype)
        vad[t] = v
        upd[t] = v < dtype(ETA)
        if upd[t]:
            lam = np.maximum(dtype(0.98) * lam + dtype(0.02) * s2, dtype(LAMBDA_MIN))
        A = xi / (dtype(1) + xi)
        if rule == 'wiener':
            G = A
        else:
            G = A * np.exp(dtype(0.5) * exp1(np.maximum(A * gam, dtype(E1_MIN)), dtype))
        P = (G * G) * s2
        o = (Ci @ (G * re) - Si @ (G * im)) / dtype(N)
        y[t * H:t * H + F] += o
    return {'y': y, 'nframes': nf, 'vad': vad, 'update': upd,
            'margin': np.abs(vad.astype(np.float64) - ETA)}


def wiener(x, srate=16000, dtype=np.float64):
    return denoise(x, srate, 'wiener', dtype)['y']


def logmmse(x, srate=16000, dtype=np.float64):
    return denoise(x, srate, 'logmmse', dtype)['y']
