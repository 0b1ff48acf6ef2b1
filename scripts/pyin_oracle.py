"""The numpy oracle of the Viterbi-smoothed pitch tracker (segan_pyin.hip, ops.pyin / ops.pyin_stages,
quality.pitch / quality.f0_eval with tracker='pyin').

pYIN (Mauch & Dixon, ICASSP 2014), written from the paper: YIN candidates under a distribution of
thresholds, then a hidden Markov model over pitch bins x {voiced, unvoiced} decoded by Viterbi.
Everything is fp64 without a transcendental function past the tables, and the decoder works on
scaled probabilities, so the device performs the same IEEE operations in the same order.

  tables      C[0..100], the running sum of the Beta(2, 18) weights of the thresholds k / 100;
              edge[0..M], the bin edges as periods in samples, descending (5 bins per semitone from
              60 Hz); A[2][2W+1], the triangular transition weights times stay / switch.
  candidates  per frame with c(tau_max + 1) > 0, YIN's pick (pitch_oracle.pick) under each of the
              100 thresholds.  The lag picked is non-increasing in the threshold, so a lag's
              thresholds form one index range (lo, hi] and its mass is C[hi] - C[lo]; the n0
              thresholds that find no lag give P_A C[n0] to the lowest lag of minimal d'.
  observation B_v(m), the masses of the candidates of bin m added in ascending lag order;
              B_u(m) = max(1 - V, 2^-40) / M with V the sum of all masses in ascending lag order.
  decoder     state j = v M + m (v = 0 voiced, 1 unvoiced); delta_0 = B_0; for t >= 1 the
              predecessors i in ascending state index over the two bands |m_i - m_j| <= W, a strictly
              larger delta_{t-1}(i) A[v_i != v_j][m_j - m_i + W] replaces the best; delta_t(j) =
              best B_t(j); after each frame delta_t times 2^-e, e the binary exponent of its maximum.
              Termination at the lowest index of maximal delta, then the backtrace.
  output      a decoded voiced state (0, m) yields the frame's candidate of bin m with the largest
              mass (lowest lag on ties); otherwise f0 = 0, lag = 0.  vprob = V.

`dtype=np.longdouble` runs the same operations in extended precision.
"""
import itertools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pitch_oracle as P  # noqa: E402

NTHETA = 100
BINS = 165
W = 11
P_A = 0.01
SWITCH = 0.01
FLOOR = 2.0 ** -40
FMIN = 60.0
BINS_PER_OCTAVE = 60


def _running(v):
    """the ascending running sums of v"""
    return np.add.accumulate(v)


def tables(srate, dtype=np.float64):
    """The constant tables as a dict: 'C' [NTHETA + 1], 'edge' [BINS + 1], 'A' [2, 2 W + 1]."""
    P.constants(srate)
    th = np.arange(NTHETA + 1).astype(dtype) / dtype(NTHETA)
    q = dtype(1) - th
    q2 = q * q
    q4 = q2 * q2
    q8 = q4 * q4
    q16 = q8 * q8
    w = th * (q16 * q)                       # theta (1 - theta)^17: Beta(2, 18) up to its constant
    tot = _running(w[1:])[-1]
    C = np.concatenate([np.zeros(1, dtype), _running(w[1:] / tot)])
    edge = dtype(srate) / (dtype(FMIN) * np.exp2(np.arange(BINS + 1).astype(dtype) /
                                                 dtype(BINS_PER_OCTAVE)))
    A = np.zeros((2, 2 * W + 1), dtype)
    for s in range(2):
        c = dtype(SWITCH) if s else dtype(1 - SWITCH)
        for k in range(-W, W + 1):
            A[s, k + W] = c * dtype(W + 1 - abs(k)) / dtype((W + 1) * (W + 1))
    return {'C': C, 'edge': edge, 'A': A}


def _as_tables(tabs, srate, dtype):
    if tabs is None:
        return tables(srate, dtype)
    return {k: np.asarray(tabs[k]).astype(dtype) for k in ('C', 'edge', 'A')}


def thresholds(dtype=np.float64):
    return np.arange(NTHETA + 1).astype(dtype) / dtype(NTHETA)


def n_at_most(v, theta):
    """how many of the thresholds theta[1 .. NTHETA] are <= v, i.e. do not have v < theta_i"""
    return int(np.searchsorted(theta[1:], v, side='right'))


def ranges(d, srate, theta):
    """The threshold index ranges of one frame's d': ({lag: (lo, hi)}, n0, the lowest lag of
    minimal d').  Thresholds lo + 1 .. hi pick the lag; thresholds 1 .. n0 find none."""
    _, tmin, tmax = P.constants(srate)
    out = {}
    hi, star, pm = NTHETA, tmin, None
    for k in range(tmin, tmax + 1):
        if pm is None or d[k] < pm:          # a new prefix minimum: the first lag below more thresholds
            pm, star = d[k], k
            lo = n_at_most(d[k], theta)
            if lo < hi:
                tau = k
                while tau < tmax and d[tau + 1] < d[tau]:
                    tau += 1
                if tau in out:
                    assert out[tau][0] == hi
                    out[tau] = (lo, out[tau][1])
                else:
                    out[tau] = (lo, hi)
                hi = lo
    return out, hi, star


def ranges_literal(d, srate, theta):
    """`ranges` by the literal loop over the thresholds, each with pitch_oracle.pick's rule."""
    _, tmin, tmax = P.constants(srate)
    picked = {}
    none = []
    for i in range(1, NTHETA + 1):
        below = np.nonzero(d[tmin:tmax + 1] < theta[i])[0]
        if not len(below):
            none.append(i)
            continue
        tau = tmin + int(below[0])
        while tau < tmax and d[tau + 1] < d[tau]:
            tau += 1
        picked.setdefault(tau, []).append(i)
    win = d[tmin:tmax + 1]
    return picked, none, tmin + int(np.argmin(win))


def ranges_by_stops(d, srate, theta):
    """`ranges` the way the kernel finds them, without a walk per prefix minimum: a descent stops
    at k = tau_max or where d'(k + 1) < d'(k) fails; with pm(k) the minimum of d' over tau_min .. k,
    the thresholds that stop at k are those above pm(k) and at most pm(the stop before k)."""
    _, tmin, tmax = P.constants(srate)
    win = np.asarray(d[tmin:tmax + 2])
    pm = np.minimum.accumulate(win[:-1])
    stop = ~(win[1:] < win[:-1])
    stop[-1] = True
    out, hi = {}, NTHETA
    for k in np.nonzero(stop)[0]:
        lo = n_at_most(pm[k], theta)
        if lo < hi:
            out[tmin + int(k)] = (lo, hi)
        hi = lo
    return out, hi, tmin + int(np.argmin(win[:-1]))


def period(d, tau, dtype=np.float64):
    """tau + delta with pitch_oracle.pick's parabola"""
    a, b, c = d[tau - 1], d[tau], d[tau + 1]
    den = a - dtype(2) * b + c
    delta = dtype(0)
    if den > 0:
        delta = dtype(0.5) * (a - c) / den
        delta = min(max(delta, dtype(-0.5)), dtype(0.5))
    return dtype(tau) + delta


def bin_of(p, edge):
    m = int((edge >= p).sum()) - 1
    return min(max(m, 0), BINS - 1)


def candidates(d, ctot, srate, tabs, theta, dtype=np.float64):
    """One frame's candidates in ascending lag order: a list of (lag, period, bin, mass)."""
    if not ctot > 0:
        return []
    rg, n0, star = ranges(d, srate, theta)
    C = tabs['C']
    mass = {tau: C[hi] - C[lo] for tau, (lo, hi) in rg.items()}
    if n0 > 0:
        mass[star] = mass.get(star, dtype(0)) + dtype(P_A) * C[n0]
    out = []
    for tau in sorted(mass):
        if mass[tau] > 0:
            p = period(d, tau, dtype)
            out.append((tau, p, bin_of(p, tabs['edge']), mass[tau]))
    return out


def observe(cands, dtype=np.float64):
    """(B [2 BINS], V) of one frame's candidates"""
    B = np.zeros(2 * BINS, dtype)
    V = dtype(0)
    for _, _, m, mass in cands:
        B[m] = B[m] + mass
        V = V + mass
    U = max(dtype(1) - V, dtype(FLOOR))
    B[BINS:] = U / dtype(BINS)
    return B, V


def viterbi(B, A, W, dtype=np.float64):
    """The banded Viterbi decoder at any M: B [F, 2 M] (voiced bins, then unvoiced), A [2, 2 W + 1].
    Returns (path [F] of state indices, the last frame's scaled delta [2 M], the smallest relative
    gap between winner and runner-up over the decisions on the decoded path, exact ties excluded;
    inf without such a decision)."""
    B = np.asarray(B, dtype)
    A = np.asarray(A, dtype)
    F, S = B.shape
    M = S // 2
    if F == 0:
        return np.zeros(0, np.int32), np.zeros(S, dtype), np.inf
    j = np.arange(S)
    vj, mj = j // M, j % M

    def rescale(dl):
        e = np.frexp(dl.max())[1]
        return np.ldexp(dl, -int(e))

    delta = rescale(B[0].copy())
    psi = np.zeros((F, S), np.int32)
    gaps = np.full((F, S), np.inf)
    for t in range(1, F):
        best = np.full(S, -1, dtype)
        second = np.full(S, -1, dtype)
        arg = np.zeros(S, np.int32)
        for vi in range(2):
            for k in range(-W, W + 1):
                mi = mj + k
                ok = (mi >= 0) & (mi < M)
                i = vi * M + np.where(ok, mi, 0)
                val = delta[i] * A[(vi != vj).astype(int), W - k]
                up = ok & (val > best)
                mid = ok & ~up & (val < best) & (val > second)
                second = np.where(up, best, np.where(mid, val, second))
                best = np.where(up, val, best)
                arg = np.where(up, i, arg).astype(np.int32)
        psi[t] = arg
        with np.errstate(divide='ignore', invalid='ignore'):
            gaps[t] = np.where((second >= 0) & (best > 0), (best - second) / best, np.inf)
        delta = rescale(best * B[t])
    path = np.zeros(F, np.int32)
    top = delta.max()
    path[F - 1] = int(np.nonzero(delta == top)[0][0])
    gap = np.inf
    rest = delta[delta < top]
    if len(rest) and top > 0:
        gap = float((top - rest.max()) / top)
    for t in range(F - 1, 0, -1):
        gap = min(gap, float(gaps[t, path[t]]))
        path[t - 1] = psi[t, path[t]]
    return path, delta, gap


def viterbi_exhaustive(B, A, W, dtype=np.float64):
    """The best path by enumerating all of them (tiny models only): the value of a path is the
    product in the decoder's own order, and among paths of equal value the one whose last state is
    lowest wins, then the one before it, and so on."""
    B = np.asarray(B, dtype)
    F, S = B.shape
    M = S // 2
    best, arg = None, None
    for path in itertools.product(range(S), repeat=F):
        v = B[0, path[0]]
        ok = True
        for t in range(1, F):
            i, j = path[t - 1], path[t]
            k = j % M - i % M
            if abs(k) > W:
                ok = False
                break
            v = (v * A[int(i // M != j // M), k + W]) * B[t, j]
        if not ok:
            continue
        key = tuple(reversed(path))
        if best is None or v > best or (v == best and key < arg):
            best, arg = v, key
    return np.asarray(tuple(reversed(arg)), np.int32), best


def track(x, srate=16000, tabs=None, dtype=np.float64):
    """The decoded contour of the row x (fp32 samples) as a dict: f0 [nf], lag [nf] int32, vprob
    [nf], bv [nf, BINS], state [nf] int32, delta [2 BINS] (the last frame's, scaled; NaN without a
    frame), gap (see `viterbi`) and cands (a list per frame).  `tabs`: the tables to use (the
    library's, in the parity tests), this module's own without."""
    x = np.asarray(x)
    if x.dtype != np.float32 or x.ndim != 1:
        raise ValueError('pyin: x must be a float32 vector')
    tabs = _as_tables(tabs, srate, dtype)
    theta = thresholds(dtype)
    dp, _, ctot = P.cmnd(x, srate, dtype)
    nf = dp.shape[0]
    cands = [candidates(dp[t], ctot[t], srate, tabs, theta, dtype) for t in range(nf)]
    B = np.zeros((nf, 2 * BINS), dtype)
    V = np.zeros(nf, dtype)
    for t in range(nf):
        B[t], V[t] = observe(cands[t], dtype)
    path, delta, gap = viterbi(B, tabs['A'], W, dtype)
    f0 = np.zeros(nf, dtype)
    lag = np.zeros(nf, np.int32)
    for t in range(nf):
        if path[t] < BINS:
            own = [c for c in cands[t] if c[2] == path[t]]
            assert own, 'a decoded voiced state without a candidate'
            top = max(c[3] for c in own)
            tau, p = next((c[0], c[1]) for c in own if c[3] == top)
            f0[t], lag[t] = dtype(srate) / p, tau
    if nf == 0:
        delta = np.full(2 * BINS, np.nan, dtype)
    return {'f0': f0, 'lag': lag, 'vprob': V, 'bv': B[:, :BINS].copy(), 'state': path,
            'delta': delta, 'gap': gap, 'cands': cands}
