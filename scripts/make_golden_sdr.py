"""Writes tests/golden/sdr.pt: the fixture of ops.sdr / ops.sdr_stages / quality.sdr, computed
with the fp64 numpy oracle scripts/sdr_oracle.py.

    python scripts/make_golden_sdr.py [out.pt]

The fixture stores no signals: every case names a track, a noise track and a gain of
tests/golden/quality.pt by key and a slice of them (`CASES`); `case_signals(qfx, name)` rebuilds
the pair (clean, optionally through the 3-tap filter h = delta_0 + 0.5 delta_7 - 0.3 delta_39,
+ gain * noise, rounded to float32 once).  Stored per case and per taps in TAPS: the SDR, r, d,
c, the order reached, St and Ee; and in `meta` what the tolerance of the GPU tests rests on:

  * solver_gap_db: the largest |SDR(Levinson) - SDR(numpy.linalg.lstsq on Toeplitz(r))| over all
    cases and taps, asserted < 1e-10 dB (the GPU tests assert 1e-8 dB);
  * definition_gap_db: the largest |SDR(taps = 16) - SDR(least squares on the explicit delay
    matrix S)|, asserted < 1e-8 dB.

It asserts too that every stored SDR is finite and below 60 dB, that every recursion reaches its
full order, that SNR 0 / 10 / 20 dB are ordered at every taps, and that the filtered case gains
more than 3 dB from 512 taps over 1.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sdr_oracle as O  # noqa: E402

TAPS = (1, 2, 33, 512)
DEFINITION_TAPS = 16
FILTER = ((0, 1.0), (7, 0.5), (39, -0.3))
ZERO_RUN = (20000, 22000)     # quality.pt's zero_run recipe: exact zeros in the clean signal
# every length is at most 3 spans of 4096 samples
CASES = {
    'snr0': dict(gain='snr0', start=0, len=12288),
    'snr10': dict(gain='snr10', start=0, len=12288),
    'snr20': dict(gain='snr20', start=0, len=12288),
    'filtered': dict(gain='snr20', start=8000, len=10000, filtered=True),
    'zero_run': dict(gain='snr10', start=16000, len=12000, zero_ref=ZERO_RUN),
    'short': dict(gain='snr10', start=9000, len=700),
    'tiny': dict(gain='snr10', start=9000, len=300),      # fewer samples than taps
}
SOLVER_GAP_LIMIT = 1e-10
DEFINITION_GAP_LIMIT = 1e-8


def case_signals(qfx, name, cases=CASES):
    """(ref, deg) of case `name`, float32, from quality.pt's signals and gains."""
    rc = cases[name]
    clean = qfx['signals']['clean'].numpy()
    noise = qfx['signals']['noise'].numpy().astype(np.float64)
    target = np.zeros(len(clean))
    for delay, h in (FILTER if rc.get('filtered') else FILTER[:1]):
        target[delay:] += h * clean[:len(clean) - delay].astype(np.float64)
    deg = (target + float(qfx['gains'][rc['gain']]) * noise).astype(np.float32)
    ref = clean.copy()
    if 'zero_ref' in rc:
        a, b = rc['zero_ref']
        ref[a:b] = 0
    sl = slice(rc['start'], rc['start'] + rc['len'])
    return ref[sl], deg[sl]


def evaluate(ref, deg, taps):
    return O.sdr_stages(ref, deg, taps)


def main(out):
    import torch
    qfx = torch.load(os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'quality.pt'),
                     map_location='cpu', weights_only=False)
    results, solver_gap, definition_gap = {}, 0.0, 0.0
    for name in CASES:
        ref, deg = case_signals(qfx, name)
        results[name] = {}
        for taps in TAPS:
            r = evaluate(ref, deg, taps)
            assert math.isfinite(r['sdr']) and r['sdr'] < 60.0, (name, taps, r['sdr'])
            assert r['order'] == taps, (name, taps, r['order'])
            solver_gap = max(solver_gap, abs(r['sdr'] - O.sdr_lstsq(ref, deg, taps)))
            results[name][taps] = {k: (torch.from_numpy(v.copy()) if isinstance(v, np.ndarray)
                                       else v) for k, v in r.items()}
        definition_gap = max(definition_gap, abs(O.sdr(ref, deg, DEFINITION_TAPS) -
                                                 O.sdr_delay_matrix(ref, deg, DEFINITION_TAPS)))
    assert solver_gap < SOLVER_GAP_LIMIT, solver_gap
    assert definition_gap < DEFINITION_GAP_LIMIT, definition_gap
    for taps in TAPS:
        v = [results[n][taps]['sdr'] for n in ('snr0', 'snr10', 'snr20')]
        assert v[0] < v[1] < v[2], (taps, v)
    assert results['filtered'][512]['sdr'] > results['filtered'][1]['sdr'] + 3.0

    fx = {'cases': CASES, 'taps': TAPS, 'results': results,
          'meta': {'recipe': 'scripts/make_golden_sdr.py', 'oracle': 'scripts/sdr_oracle.py',
                   'signals': 'tests/golden/quality.pt', 'solver_gap_db': solver_gap,
                   'definition_gap_db': definition_gap, 'definition_taps': DEFINITION_TAPS,
                   'numpy': np.__version__}}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')
    for n in CASES:
        print('  {:9s} L = {:5d}  SDR ='.format(n, CASES[n]['len']) + ''.join(
            '  {:.9f} ({} taps)'.format(results[n][t]['sdr'], t) for t in TAPS))
    print('  solver_gap_db', solver_gap, ' definition_gap_db', definition_gap)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'sdr.pt'))
