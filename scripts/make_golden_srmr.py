"""Writes tests/golden/srmr.pt: the fixture of ops.srmr / ops.srmr_stages / quality.srmr, computed
with the fp64 numpy / scipy oracle scripts/srmr_oracle.py.

    python scripts/make_golden_srmr.py [out.pt]

The fixture stores no signals: every case names a slice of the clean track of
tests/golden/quality.pt, optionally a noise gain of that file, optionally the synthetic room
response built here (`impulse_response`: seeded white noise under an exponential decay with
RT60 = 0.4 s after a direct path of 1), and `case_signal(qfx, name)` rebuilds the row (rounded to
float32 once).  Stored per case: cfs, envelope_energy, energy (Ebar), share, bw, kstar, srmr; and
in `meta` what the tolerance of the GPU tests rests on:

  * oracle_gap: the largest relative difference in SRMR and in any Ebar[i, k] between the oracle
    in float64 and the same oracle with filters and sums in numpy.longdouble;
  * definition_gap: the largest |SRMR(padded to a power of two) - SRMR(Hilbert transform of
    exactly N samples, as the toolbox does)|: reported, not asserted.

It asserts that every stored SRMR is finite, that the reverberant case scores lower than its dry
source, and that in every case the cumulated share that decides BW is further than 1e-6 from 90,
so that K* cannot flip on rounding.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import srmr_oracle as O  # noqa: E402

RATE = 16000
RIR = dict(seed=20260, rt60=0.4, taps=4000, level=0.25)
# every length is at most 12305 samples
CASES = {
    'dry': dict(start=0, len=12305),
    'reverberant': dict(start=0, len=12305, reverb=True),
    'snr0': dict(start=3000, len=12288, gain='snr0'),
    'snr20': dict(start=3000, len=12288, gain='snr20'),
    'n4096': dict(start=9000, len=4096),
    'n4097': dict(start=9000, len=4097),
}
SHARE_MARGIN = 1e-6


def impulse_response():
    """The synthetic room response: h[0] = 1, then level * noise * 10^(-3 t / rt60)."""
    rng = np.random.default_rng(RIR['seed'])
    t = np.arange(RIR['taps']) / RATE
    h = RIR['level'] * rng.standard_normal(RIR['taps']) * 10.0 ** (-3.0 * t / RIR['rt60'])
    h[0] = 1.0
    return h


def case_signal(qfx, name, cases=CASES):
    """The float32 row of case `name`, from quality.pt's signals and gains."""
    rc = cases[name]
    clean = qfx['signals']['clean'].numpy().astype(np.float64)
    x = clean
    if rc.get('reverb'):
        x = np.convolve(clean, impulse_response())[:len(clean)]
        x = x * (np.abs(clean).max() / np.abs(x).max())
    if 'gain' in rc:
        x = x + float(qfx['gains'][rc['gain']]) * qfx['signals']['noise'].numpy().astype(np.float64)
    return x.astype(np.float32)[rc['start']:rc['start'] + rc['len']]


def evaluate(x):
    return O.stages(x, RATE)


def rel_gap(a, b):
    """The largest relative difference in SRMR and in any Ebar[i, k] between two stage dicts."""
    g = abs(a['srmr'] - b['srmr']) / abs(b['srmr'])
    return max(g, float(np.max(np.abs(a['energy'] - b['energy']) / b['energy'])))


def main(out):
    import torch
    qfx = torch.load(os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'quality.pt'),
                     map_location='cpu', weights_only=False)
    results, oracle_gap, definition_gap = {}, 0.0, 0.0
    for name in CASES:
        x = case_signal(qfx, name)
        assert x.dtype == np.float32 and len(x) == CASES[name]['len'] <= 12305
        r = evaluate(x)
        assert math.isfinite(r['srmr']), (name, r['srmr'])
        assert abs(r['share'] - 90.0) > SHARE_MARGIN, (name, r['share'])
        ext = O.stages(x, RATE, dtype=np.longdouble)
        assert ext['kstar'] == r['kstar'] and ext['bw'] == r['bw'], name
        oracle_gap = max(oracle_gap, rel_gap(r, ext))
        definition_gap = max(definition_gap, abs(r['srmr'] - O.srmr(x, RATE, exact=True)))
        results[name] = {k: (torch.from_numpy(v.copy()) if isinstance(v, np.ndarray) else v)
                         for k, v in r.items()}
    assert results['reverberant']['srmr'] < results['dry']['srmr']
    fx = {'cases': CASES, 'rate': RATE, 'rir': RIR, 'results': results,
          'meta': {'recipe': 'scripts/make_golden_srmr.py', 'oracle': 'scripts/srmr_oracle.py',
                   'signals': 'tests/golden/quality.pt', 'oracle_gap': oracle_gap,
                   'definition_gap': definition_gap, 'share_margin': SHARE_MARGIN,
                   'numpy': np.__version__}}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')
    for n in CASES:
        r = results[n]
        print('  {:12s} N = {:5d}  SRMR = {:.12f}  K* = {}  BW = {:.3f}  share = {:.6f}'.format(
            n, CASES[n]['len'], r['srmr'], r['kstar'], r['bw'], r['share']))
    print('  oracle_gap', oracle_gap, ' definition_gap', definition_gap)


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'srmr.pt'))
