"""Writes tests/golden/resample.pt: the fixture of ops.resample, computed with the fp64 numpy oracle
scripts/resample_oracle.py.

    python scripts/make_golden_resample.py [out.pt]

Per case (rate_in, rate_out, zeros, beta): a ragged batch whose row lengths are derived from the
kernel's output tile (TILE) and the filter — 0, 1 and 2 samples, a row shorter than the filter, the
rows that yield TILE - 1, TILE and TILE + 1 outputs (or the nearest counts the ratio can produce)
and a row of more than three tiles (16000 -> 12345 Hz, whose taps fit nowhere on chip, keeps to 700
samples).  Inputs are seeded and rebuilt by `case_inputs`; stored are the seeds and the expected
outputs: fp64 of the fp32 noise rows, int16 of the int16 noise rows, int16 and saturation counts
of a full-scale square wave of period 80.  The recipe asserts that the oracle equals
scipy.signal.resample_poly, that every int16 expectation lies at least 1e-6 from a half-integer
(a case whose seeded noise
comes closer takes its next seed; the fixture therefore needs no leave-out allowance), that the noise rows never saturate and that the
square wave does on every case.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_oracle as R  # noqa: E402

TILE = 256                      # outputs per workgroup of the kernel (ops.resample_dims)
RATES = ((48000, 16000), (44100, 16000), (8000, 16000), (16000, 48000), (16000, 44100),
         (16000, 12345), (192000, 8000))
FILTERS = ((32, 8.6), (10, 5.0))
MAX_IN = {(16000, 12345): 700}  # rows of at most this many samples
SQUARE_PERIOD = 80
HALF_MARGIN = 1e-6


def cases():
    return [(a, b, z, be) for (a, b) in RATES for (z, be) in FILTERS]


def in_len_for(n_out, p, q):
    """The shortest row that yields at least n_out outputs."""
    return (n_out - 1) * q // p + 1 if n_out > 0 else 0


def row_lengths(rate_in, rate_out, zeros):
    p, q = R.ratio(rate_in, rate_out)
    lh = zeros * max(p, q)
    span = 2 * lh // p + 1                               # input samples under the filter
    lens = [0, 1, 2, max(3, span // 2)]
    lens += [in_len_for(n, p, q) for n in (TILE - 1, TILE, TILE + 1)]
    cap = MAX_IN.get((rate_in, rate_out))
    lens.append(cap if cap is not None else in_len_for(3 * TILE + 37, p, q))
    out = []
    for L in lens:
        if L not in out and (cap is None or L <= cap):
            out.append(L)
    return out


def case_seed(case, attempt=0):
    a, b, z, _ = case
    return (a * 7 + b * 3 + z) % (2 ** 31) + 1000003 * attempt


def case_inputs(case, seed=None):
    """(lens, xf fp32 [rows, T], xi int16 [rows, T], square int16 [T]) rebuilt from the seed (the
    tests pass the fixture's); the rows are zero past their lengths."""
    a, b, z, _ = case
    lens = row_lengths(a, b, z)
    T = max(lens)
    rng = np.random.default_rng(case_seed(case) if seed is None else seed)
    xf = np.zeros((len(lens), T), dtype=np.float32)
    xi = np.zeros((len(lens), T), dtype=np.int16)
    for r, L in enumerate(lens):
        xf[r, :L] = rng.standard_normal(L).astype(np.float32)
        xi[r, :L] = rng.integers(-12000, 12001, size=L).astype(np.int16)
    sq = np.where((np.arange(T) // (SQUARE_PERIOD // 2)) % 2 == 0, 32767, -32768).astype(np.int16)
    return lens, xf, xi, sq


def expected(case):
    """The first of the case's seeds whose int16 expectations keep HALF_MARGIN (the square wave,
    which no seed changes, has to keep it as it is)."""
    for attempt in range(8):
        e = expected_for(case, case_seed(case, attempt))
        if e['sq_margin'] < HALF_MARGIN or e['margin'] >= HALF_MARGIN:
            break
        print(case, 'seed', e['seed'], 'margin %.2e: next seed' % e['margin'])
    assert e['margin'] >= HALF_MARGIN, (case, e['margin'], e['sq_margin'])
    return e


def expected_for(case, seed):
    a, b, z, be = case
    p, q, taps = R.plan(a, b, z, be)
    lens, xf, xi, sq = case_inputs(case, seed)
    y64, y16 = [], []
    margin = np.inf
    for r, L in enumerate(lens):
        yf = R.resample(xf[r, :L], p, q, taps)
        yi = R.resample(xi[r, :L], p, q, taps)
        for x, y in ((xf[r, :L], yf), (xi[r, :L], yi)):
            ys = R.resample_scipy(x, p, q, taps)
            assert ys.shape == y.shape == (R.out_len(L, p, q),), (case, L)
            if L:
                assert np.abs(ys - y).max() <= 1e-12 * np.abs(y).max(), (case, L)
        margin = min(margin, R.half_distance(yi))
        i16, nclip = R.to_int16(yi)
        assert nclip == 0, (case, L, nclip)
        y64.append(yf)
        y16.append(i16)
    ysq = R.resample(sq, p, q, taps)
    sq_margin = R.half_distance(ysq)
    margin = min(margin, sq_margin)
    sq16, sq_nclip = R.to_int16(ysq)
    assert sq_nclip > 0 and np.abs(ysq).max() > 36000, (case, sq_nclip, np.abs(ysq).max())
    return dict(seed=seed, sq_margin=sq_margin, p=p, q=q, lens=lens,
                out_lens=[R.out_len(L, p, q) for L in lens],
                y64=np.concatenate(y64), y16=np.concatenate(y16), sq16=sq16, sq_nclip=sq_nclip,
                sq_peak=float(np.abs(ysq).max()), margin=margin)


def main(out):
    import torch
    fx = dict(tile=TILE, cases={})
    for case in cases():
        e = expected(case)
        print(case, 'rows', e['lens'], '->', e['out_lens'], 'square peak %.0f nclip %d margin %.2e'
              % (e['sq_peak'], e['sq_nclip'], e['margin']))
        fx['cases'][case] = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v)
                             for k, v in e.items()}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'resample.pt'))
