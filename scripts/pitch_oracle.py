"""The numpy oracle of the GPU pitch tracker and of the F0 / voicing measures (segan_pitch.hip,
ops.pitch / ops.pitch_stages / ops.f0_eval, quality.pitch / quality.f0_eval).

YIN (de Cheveigne & Kawahara 2002) with a 5 ms hop, fp64 on fp32 samples, in the kernel's own
order of operations:

  * hop blocks of H samples: S_u(tau) = sum x[j] x[j+tau], E_u(tau) = sum x[j+tau]^2, j ascending
    (the products of two fp32 values are exact in fp64, so the kernel's fused multiply-adds and
    the separate ones here give the same bits);
  * a frame is NB = 5 blocks, added in ascending order; d(tau) = (E(0) + E(tau)) - 2 R(tau);
  * c(tau) the ascending running sum of d(1 .. tau) (numpy's cumsum is sequential);
    d'(tau) = d(tau) tau / c(tau) where c(tau) > 0, else 1;
  * the pick, the parabola and f0 = srate / (tau + delta).

`dtype=np.longdouble` runs the same operations in extended precision: the movement between the
two is what the tolerances of the GPU tests are taken from.  Besides the contour every frame gets
its decision margin: the smallest |d'(k) - theta| over the lags the threshold scan looked at and
|d'(k+1) - d'(k)| over the steps (and the stop) of the descent; a frame whose margin is far above
the rounding of d' cannot flip between two implementations.
"""
import math

import numpy as np

NB = 5
THETA = 0.15
RATES = (16000, 8000)


def constants(srate):
    """(H, tau_min, tau_max) at `srate`: 80, 40, 266 at 16 kHz, halved at 8 kHz."""
    if srate not in RATES:
        raise ValueError('pitch: srate must be one of {}, got {!r}'.format(RATES, srate))
    div = 16000 // srate
    return 80 // div, 40 // div, 266 // div


def n_blocks(L, srate):
    H, _, tmax = constants(srate)
    return (L - (tmax + 1)) // H if L >= tmax + 1 else 0


def n_frames(L, srate):
    nb = n_blocks(L, srate)
    return nb - NB + 1 if nb >= NB else 0


def block_sums(x, srate, dtype=np.float64):
    """S, E [nb, tau_max + 2] of the row x (fp32 samples)."""
    H, _, tmax = constants(srate)
    x = np.asarray(x)
    nb, nl = n_blocks(len(x), srate), tmax + 2
    xd = x.astype(dtype)
    S = np.zeros((nb, nl), dtype)
    E = np.zeros((nb, nl), dtype)
    base = (np.arange(nb) * H)[:, None] + np.arange(nl)[None, :]
    for j in range(H):
        a = xd[np.arange(nb) * H + j][:, None]
        b = xd[base + j]
        S = S + a * b
        E = E + b * b
    return S, E


def cmnd(x, srate=16000, dtype=np.float64):
    """(d' [nf, tau_max + 2], the cancellation scale (E(0) + E(tau)) tau / c(tau) of each element
    [nf, tau_max + 2] (0 where d' is the constant 1), c(tau_max + 1) [nf])."""
    _, _, tmax = constants(srate)
    nl, nf = tmax + 2, n_frames(len(x), srate)
    S, E = block_sums(x, srate, dtype)
    if nf == 0:
        return np.zeros((0, nl), dtype), np.zeros((0, nl), dtype), np.zeros(0, dtype)
    R, Et = S[0:nf], E[0:nf]
    for u in range(1, NB):
        R = R + S[u:u + nf]
        Et = Et + E[u:u + nf]
    big = Et[:, :1] + Et
    d = big - dtype(2) * R
    d[:, 0] = 0
    c = np.concatenate([np.zeros((nf, 1), dtype), np.cumsum(d[:, 1:], axis=1, dtype=dtype)], axis=1)
    tau = np.arange(nl).astype(dtype)[None, :]
    pos = c > 0
    safe = np.where(pos, c, dtype(1))
    dp = np.where(pos, d * tau / safe, dtype(1))
    scale = np.where(pos, big * tau / safe, dtype(0))
    return dp, scale, c[:, -1]


def pick(dp, ctot, srate=16000, theta=THETA, dtype=np.float64):
    """The per-frame decisions on d' [nf, nl]: (f0, lag, ap, margin)."""
    _, tmin, tmax = constants(srate)
    nf = dp.shape[0]
    theta = dtype(theta)
    f0 = np.zeros(nf, dtype)
    lag = np.zeros(nf, np.int32)
    ap = np.zeros(nf, dtype)
    margin = np.full(nf, np.inf)
    for t in range(nf):
        d = dp[t]
        tau = 0
        if ctot[t] > 0:
            win = d[tmin:tmax + 1]
            below = np.nonzero(win < theta)[0]
            last = below[0] if len(below) else len(win) - 1
            m = float(np.min(np.abs(win[:last + 1] - theta)))
            if len(below):
                tau = tmin + int(below[0])
                while tau < tmax:
                    m = min(m, float(abs(d[tau + 1] - d[tau])))
                    if not d[tau + 1] < d[tau]:
                        break
                    tau += 1
            margin[t] = m
        if tau:
            a, b, c = d[tau - 1], d[tau], d[tau + 1]
            den = a - dtype(2) * b + c
            delta = dtype(0)
            if den > 0:
                delta = dtype(0.5) * (a - c) / den
                delta = min(max(delta, dtype(-0.5)), dtype(0.5))
            f0[t] = dtype(srate) / (dtype(tau) + delta)
            ap[t] = b
        else:
            ap[t] = np.min(d[tmin:tmax + 1])
        lag[t] = tau
    return f0, lag, ap, margin


def track(x, srate=16000, theta=THETA, dtype=np.float64):
    """The contour of the row x (fp32 samples) as a dict: f0 [nf] (0 when unvoiced), lag [nf]
    int32 (0 when unvoiced), ap [nf], margin [nf] (the decision margin, inf for a frame without
    energy), cmnd and scale [nf, tau_max + 2]."""
    if not 0 < theta <= 1:
        raise ValueError('pitch: the threshold must lie in (0, 1], got {!r}'.format(theta))
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 1:
        raise ValueError('pitch: x must be a float32 vector')
    dp, scale, ctot = cmnd(x, srate, dtype)
    f0, lag, ap, margin = pick(dp, ctot, srate, theta, dtype)
    return {'f0': f0, 'lag': lag, 'ap': ap, 'margin': margin, 'cmnd': dp, 'scale': scale}


def contour(f0, lag, dtype=np.float64):
    """log f0 at the voiced frames (lag > 0), elsewhere on the line between the neighbouring voiced
    frames p < t < n, lp + (t - p) ((ln - lp) / (n - p)), before the first and after the last
    voiced frame the nearest one's.  Needs a voiced frame."""
    f0 = np.asarray(f0, dtype)
    idx = np.nonzero(np.asarray(lag) > 0)[0]
    l = np.zeros(len(f0), dtype)
    lv = np.log(f0[idx])
    for t in range(len(f0)):
        k = int(np.searchsorted(idx, t))           # idx[k - 1] < t <= idx[k]
        if k < len(idx) and idx[k] == t:
            l[t] = lv[k]
        elif k == 0:
            l[t] = lv[0]
        elif k == len(idx):
            l[t] = lv[-1]
        else:
            p, n = int(idx[k - 1]), int(idx[k])
            l[t] = lv[k - 1] + dtype(t - p) * ((lv[k] - lv[k - 1]) / dtype(n - p))
    return l


def _sum(v, dtype):
    """The sum of v in ascending order."""
    return np.add.accumulate(np.asarray(v, dtype))[-1] if len(v) else dtype(0)


def f0_eval(f0_ref, lag_ref, f0_deg, lag_deg, dtype=np.float64):
    """The measures on two contours of nf common frames, as a dict of floats: f0_mae (Hz, over
    the reference's voiced frames), vuv_acc, f0_kld, voiced; NaN by the rules of DESIGN.md
    section 19."""
    nf = len(f0_ref)
    nan = dtype(math.nan)
    out = {'f0_mae': nan, 'vuv_acc': nan, 'f0_kld': nan, 'voiced': nan}
    if nf == 0:
        return out
    ur, ud = np.asarray(lag_ref) > 0, np.asarray(lag_deg) > 0
    out['vuv_acc'] = dtype(int((ur == ud).sum())) / dtype(nf)
    out['voiced'] = dtype(int(ur.sum())) / dtype(nf)
    if not ur.any() or not ud.any():
        return out
    lr, ld = contour(f0_ref, lag_ref, dtype), contour(f0_deg, lag_deg, dtype)
    out['f0_mae'] = _sum(np.where(ur, np.abs(np.exp(ld) - np.exp(lr)), dtype(0)), dtype) / dtype(
        int(ur.sum()))
    mr, md = _sum(lr, dtype) / dtype(nf), _sum(ld, dtype) / dtype(nf)
    if nf >= 2:
        sg = np.sqrt(_sum((lr - mr) * (lr - mr), dtype) / dtype(nf - 1))
        sp = np.sqrt(_sum((ld - md) * (ld - md), dtype) / dtype(nf - 1))
        if sp != 0:
            dm = md - mr
            with np.errstate(divide='ignore'):
                out['f0_kld'] = (np.log(sg / sp + dtype(1e-22)) +
                                 (sp * sp + dm * dm) / (dtype(2) * (sg * sg) + dtype(1e-22)) -
                                 dtype(0.5))
    return out


def evaluate(ref, deg, srate=16000, theta=THETA, dtype=np.float64):
    """f0_eval of the contours of two rows of the same length."""
    if len(ref) != len(deg):
        raise ValueError('f0_eval: ref and deg differ in length')
    a, b = track(ref, srate, theta, dtype), track(deg, srate, theta, dtype)
    return f0_eval(a['f0'], a['lag'], b['f0'], b['lag'], dtype)
