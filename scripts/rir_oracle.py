"""The numpy oracle of the room-impulse-response synthesis: the definition
that segan_rir.hip and ops.rir_shoebox implement.

The image-source method for a shoebox room (Allen & Berkley, JASA 65, 1979) with Peterson's
low-pass impulse for the fractional delays (Peterson, JASA 80, 1986: a Hann-windowed sinc of 8 ms),
written from the two papers.  Nothing else is modelled: no high-pass filter, no microphone
directivity, no air absorption, no diffuse tail.

Per response: the room L[3] in metres, the source s[3] and the receiver r[3] strictly inside it,
beta[6] in [0, 1], the reflection coefficients of the walls x = 0, x = Lx, y = 0, y = Ly, z = 0,
z = Lz, the rate srate (16000 or 8000), c = 343 m/s, the length T and the half-width
Hw = srate / 250 samples.

Images.  For (n, l, m) in Z^3 and (q, j, k) in {0, 1}^3, every product and sum rounded on its own:

    px = ((1 - 2 q) sx - rx) + (2 n) Lx,  py and pz alike
    d = sqrt((px^2 + py^2) + pz^2)
    tau = d (srate / c)
    a = (((bx0^|n - q| bx1^|n|) (by0^|l - j| by1^|l|)) (bz0^|m - k| bz1^|m|)) / ((4 pi) d)

The powers are read from the tables of `ops.rir_tables`: tab[w][0] = 1, tab[w][i] = tab[w][i - 1]
beta_w, so 0^0 = 1 and beta = 0 leaves the direct path alone.  The device reads the same bits.

Contribution.  n0 = floor(tau), f = tau - n0 (exact), and for every integer k' with
|k' - f| < Hw the sample t = n0 + k', 0 <= t < T, receives

    (a (0.5 (1 + cos(pi (k' - f) / Hw)))) sinc,   sinc = -(-1)^k' sin(pi f) / (pi (k' - f)),

sinc = 1 where k' - f = 0.  This is sin(pi (t - tau)) / (pi (t - tau)) with the integer part of the
argument reduced away, so the error of the argument does not grow with tau.

The image set is every image that reaches a sample below T, that is n0 - Hw + 1 <= T - 1; `images`
counts them, whatever their amplitude.  The enumeration below is a superset, and a superset gives
the same response: the window vanishes at its edge, so there is no decision in the definition.

`rir` runs unchanged in numpy.longdouble (`dtype=`); the movement between the two runs is what the
tolerances of the GPU test are made of (scripts/make_golden_rir.py).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C = 343.0
RATES = (16000, 8000)


def half_width(srate):
    if srate not in RATES:
        raise ValueError('rir: srate must be one of {}, got {!r}'.format(RATES, srate))
    return srate // 250


def tables(beta, n_max):
    """ops.rir_tables: the one builder, so that oracle and device read the same bits."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from segan_pytorch_amd import ops
    return ops.rir_tables(beta, n_max)


def _axis(L, s, r, dmax, dtype):
    """every image of one axis with |p| <= dmax, and one more on each side: n, q, p"""
    N = int(np.floor(float(dmax) / (2.0 * float(L)))) + 2
    n = np.repeat(np.arange(-N, N + 1), 2)
    q = np.tile(np.array([0, 1]), 2 * N + 1)
    p = ((1 - 2 * q) * dtype(s) - dtype(r)) + (2 * n) * dtype(L)
    return n, q, p


def rir(L, s, r, beta, T, srate=16000, dtype=np.float64, tab=None):
    """The response of one room: dict(h [T] of `dtype`, images, margin).  `margin` is the smallest
    |tau - (T + Hw - 1)| over the enumerated images, in samples: how far the closest image is from
    changing `images`.  `tab`: the power tables [6, >= n_max + 1] (built here when None)."""
    Hw = half_width(srate)
    L, s, r, beta = (np.asarray(v, np.float64).reshape(-1) for v in (L, s, r, beta))
    if L.shape != (3,) or s.shape != (3,) or r.shape != (3,) or beta.shape != (6,):
        raise ValueError('rir: L, s, r are 3 numbers and beta 6')
    T = int(T)
    rate = dtype(srate) / dtype(C)
    dmax = dtype(T + Hw + 1) / rate
    ax = [_axis(L[w], s[w], r[w], dmax, dtype) for w in range(3)]
    n_max = max(int(np.abs(a[0]).max()) for a in ax) + 1
    if tab is None:
        tab = tables(beta, n_max)[0]
    tab = np.asarray(tab).astype(dtype)
    amp = [tab[2 * w][np.abs(n - q)] * tab[2 * w + 1][np.abs(n)] for w, (n, q, _) in enumerate(ax)]
    (_, _, px), (_, _, py), (_, _, pz) = ax
    pi = dtype(np.pi)
    kp = np.arange(-Hw + 1, Hw + 1)
    sign = np.where(kp % 2 == 0, -1, 1).astype(dtype)     # -(-1)^k'
    h = np.zeros(T, dtype)
    images, margin = 0, np.inf
    pz2 = pz * pz
    for ix in range(len(px)):
        rho2 = (px[ix] * px[ix] + py * py)[:, None]
        d = np.sqrt(rho2 + pz2[None, :])
        tau = d * rate
        n0 = np.floor(tau)
        margin = min(margin, float(np.abs(tau - dtype(T + Hw - 1)).min()))
        sel = n0 - Hw + 1 <= T - 1
        images += int(sel.sum())
        if not sel.any():
            continue
        a = ((amp[0][ix] * amp[1])[:, None] * amp[2][None, :])[sel] / ((dtype(4) * pi) * d[sel])
        tau, n0 = tau[sel], n0[sel]
        f = tau - n0
        x = kp[None, :].astype(dtype) - f[:, None]
        t = n0.astype(np.int64)[:, None] + kp[None, :]
        ok = (np.abs(x) < Hw) & (t >= 0) & (t < T)
        zero = x == 0
        with np.errstate(divide='ignore', invalid='ignore'):
            sinc = (sign[None, :] * np.sin(pi * f)[:, None]) / (pi * x)
        sinc[zero] = 1
        v = (a[:, None] * (dtype(0.5) * (1 + np.cos(pi * x / Hw)))) * sinc
        if dtype is np.float64:
            h += np.bincount(t[ok], weights=v[ok], minlength=T)
        else:
            np.add.at(h, t[ok], v[ok])
    return dict(h=h, images=images, margin=margin)


def rir_rows(geom, T, srate=16000, lengths=None, dtype=np.float64):
    """`rir` for every row of geom [count, 15] = L, s, r, beta: dict(h [count, T], images [count],
    margin [count]); row i is computed at its own length lengths[i] and zero from there on."""
    geom = np.asarray(geom, np.float64).reshape(-1, 15)
    h = np.zeros((len(geom), T), dtype)
    images, margin = np.zeros(len(geom), np.int64), np.zeros(len(geom))
    for i, g in enumerate(geom):
        Li = T if lengths is None else int(lengths[i])
        if Li > 0:
            o = rir(g[0:3], g[3:6], g[6:9], g[9:15], Li, srate, dtype)
            h[i, :Li], images[i], margin[i] = o['h'], o['images'], o['margin']
        else:
            margin[i] = np.inf
    return dict(h=h, images=images, margin=margin)


def schroeder_t30(h, srate):
    """The reverberation time from the backward-integrated energy decay (Schroeder 1965): twice the
    time the decay takes from -5 to -35 dB, by a least-squares line through that stretch."""
    e = np.cumsum(np.asarray(h, np.float64)[::-1] ** 2)[::-1]
    db = 10.0 * np.log10(e / e[0] + 1e-300)
    i0 = int(np.argmax(db <= -5.0))
    i1 = int(np.argmax(db <= -35.0))
    if i1 <= i0:
        raise ValueError('schroeder_t30: the response does not decay by 35 dB')
    t = np.arange(i0, i1) / float(srate)
    slope = np.polyfit(t, db[i0:i1], 1)[0]
    return -60.0 / slope
