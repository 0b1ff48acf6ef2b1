"""fp64 numpy oracle of ESTOI, Jensen & Taal's extended short-time objective intelligibility
("ESTOI", states the rules it follows).  It checks the HIP kernel behind
ops.estoi: scripts/make_golden_estoi.py runs it to write tests/golden/estoi.pt, and
tests/test_estoi.py runs it again against that fixture.  Everything up to the band envelopes is
stoi_oracle's; only the last stage is here, written as array operations over all segments at once.

    import estoi_oracle as E
    d = E.estoi(clean, processed, 16000)          # float, NaN where ESTOI is undefined
    st = E.estoi_stages(clean, processed, 16000)   # every intermediate as a dict

The zero rule: a vector v (a band over a window's 30 frames, then a frame over the 15 bands of the
row-normalised window) becomes (v - mean v) / ||v - mean v|| when sum v^2 > 0 and
||v - mean v||^2 > 2^-40 sum v^2, and zeros otherwise.  Jensen's MATLAB adds eps * randn before
each normalisation instead; the zero rule is deterministic and is what that noise does on average:
a degenerate vector correlates with nothing.
"""
import math

import numpy as np

import stoi_oracle as S

SEG = S.SEG
J = S.J
ZERO_RULE = 2.0 ** -40      # a vector is kept when e > ZERO_RULE * raw
MARGIN = (2.0 ** -80, 2.0 ** -20)   # no e / raw of a fixture case may lie in here


def windows(X):
    """[S, J, SEG] view of the segments X[:, s:s+SEG] of the band envelopes X [J, F']."""
    if X.shape[1] < SEG:
        return np.zeros((0, J, SEG))
    return np.lib.stride_tricks.sliding_window_view(X, SEG, axis=1).transpose(1, 0, 2)


def normalise(W, axis):
    """The zero rule along `axis` of W.  Returns (normalised W, e / raw of every vector with
    raw > 0 as a flat array, number of vectors zeroed)."""
    raw = np.sum(W * W, axis=axis, keepdims=True)
    c = W - np.mean(W, axis=axis, keepdims=True)
    e = np.sum(c * c, axis=axis, keepdims=True)
    keep = (raw > 0) & (e > ZERO_RULE * raw)
    out = np.where(keep, c / np.sqrt(np.where(keep, e, 1.0)), 0.0)
    ratios = (e[raw > 0] / raw[raw > 0]).ravel()
    return out, ratios, int(keep.size - np.count_nonzero(keep))


def segment_values(X, Y):
    """(dm [S], ratios, zeroed): d_s of every segment of the band envelopes X, Y [J, F'], the
    e / raw of every normalised vector (rows and columns, both signals) and how many vectors the
    zero rule dropped."""
    ratios, zeroed = [], 0
    N = []
    for W in (windows(X), windows(Y)):
        for axis in (2, 1):     # rows: each band over the frames; then columns: each frame over the bands
            W, r, z = normalise(W, axis)
            ratios.append(r)
            zeroed += z
        N.append(W)
    dm = np.einsum('sjf,sjf->s', N[0], N[1]) / SEG
    return dm, np.concatenate(ratios), zeroed


def segment_value_loops(Xs, Ys):
    """d_s of one pair of windows [J, SEG] by literal per-element loops (the array form's check)."""
    def norm(vec):
        raw = 0.0
        for v in vec:
            raw += v * v
        mean = 0.0
        for v in vec:
            mean += v
        mean /= len(vec)
        e = 0.0
        for v in vec:
            e += (v - mean) * (v - mean)
        if raw > 0 and e > ZERO_RULE * raw:
            return [(v - mean) / math.sqrt(e) for v in vec]
        return [0.0] * len(vec)

    out = []
    for W in (Xs, Ys):
        rows = [norm([float(W[i][f]) for f in range(SEG)]) for i in range(J)]
        cols = [norm([rows[i][f] for i in range(J)]) for f in range(SEG)]
        out.append(cols)      # [SEG][J]
    acc = 0.0
    for f in range(SEG):
        for i in range(J):
            acc += out[0][f][i] * out[1][f][i]
    return acc / SEG


def margin_ok(ratios):
    """True when no e / raw lies in MARGIN: the kernel's and the oracle's keep / drop decisions
    then cannot differ through summation order."""
    return not np.any((ratios >= MARGIN[0]) & (ratios <= MARGIN[1]))


def estoi_stages(x, y, srate):
    """STOI's stages (stoi_oracle.stoi_stages) with dm [S] in place of rho, ESTOI's d, and the
    zero rule's record: ratios (e / raw of every vector), zeroed (vectors dropped)."""
    st = S.stoi_stages(x, y, srate)
    del st['rho']
    dm, ratios, zeroed = segment_values(st['X'], st['Y'])
    st.update(dm=dm, ratios=ratios, zeroed=zeroed,
              d=float(np.mean(dm)) if st['M'] and dm.size else math.nan)
    return st


def estoi(x, y, srate):
    """ESTOI of the clean x and the processed y: float in [-1, 1], NaN when the clean signal has
    no frame above -inf dB or fewer than 30 band frames remain."""
    return estoi_stages(x, y, srate)['d']
