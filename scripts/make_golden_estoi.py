"""Writes tests/golden/estoi.pt: the ESTOI fixture of ops.estoi / quality.estoi, computed with the
fp64 numpy oracle scripts/estoi_oracle.py ("ESTOI").

    python scripts/make_golden_estoi.py [out.pt]

The fixture stores no signals: every case is a case of tests/golden/stoi.pt, or one of three more
slices of its clean / noise tracks (`extra_cases`: the stage16k track from sample 8000 at its 0 dB
gain, cut to the shortest multiple of 64 samples that keeps M = 30, 31 and 32 frames: no segment,
one, two).  `case_signals(sfx, efx, name)` rebuilds a case from the two fixtures.  Stored: d of
every case, dm of the stage cases, zero_run and the one- and two-segment slices, the zero rule's
record of zero_run, and ESTOI of stoi.pt's three eval-CLI wav pairs.  The recipe asserts that
no e / raw of any case lies in [2^-80, 2^-20] (the zero rule's threshold 2^-40 sits in the middle
of that gap, so a different summation order cannot change a keep / drop decision), that zero_run
does drop vectors, and that d is strictly monotone in the SNR.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import estoi_oracle as E  # noqa: E402
import make_golden_stoi as G  # noqa: E402
import stoi_oracle as S  # noqa: E402

SLICE_START = 8000
SLICE_STEP = 64
SLICES = (('m30', 30), ('m31', 31), ('m32', 32))     # name, kept frames M
DM_CASES = ('stage16k', 'stage8k', 'zero_run', 'm31', 'm32')


def case_signals(sfx, efx, name):
    """(ref, deg, srate) of case `name`: stoi.pt's own (make_golden_stoi.case_signals), or one of
    estoi.pt's extra slices of stoi.pt's tracks."""
    if name in efx['extra_cases']:
        sfx = {'signals': sfx['signals'], 'cases': efx['extra_cases']}
    return G.case_signals(sfx, name)


def kept_frames(ref, deg, srate):
    p, q, taps = S.plan(srate)
    return S.remove_silent_frames(S.resample(ref, p, q, taps), S.resample(deg, p, q, taps))[2]


def find_slices(sfx):
    """The shortest lengths (multiples of SLICE_STEP) from SLICE_START of the stage16k track
    with M = 30, 31, 32."""
    base = sfx['cases']['stage16k']
    total = sfx['signals']['clean'].numel()
    found, want = {}, dict((m, n) for n, m in SLICES)
    L = SLICE_STEP
    while len(found) < len(want) and SLICE_START + L <= total:
        rc = dict(srate=base['srate'], start=SLICE_START, len=L, gain=base['gain'])
        M = kept_frames(*G.case_signals({'signals': sfx['signals'], 'cases': {'c': rc}}, 'c'))
        if M in want and want[M] not in found:
            found[want[M]] = rc
        L += SLICE_STEP
    assert len(found) == len(want), found
    return found


def main(out):
    import torch
    sfx = torch.load(os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'stoi.pt'),
                     map_location='cpu', weights_only=False)
    efx = {'extra_cases': find_slices(sfx)}
    names = list(sfx['cases']) + [n for n, _ in SLICES]

    d, dm, M, ratio_gap = {}, {}, {}, {}
    for name in names:
        ref, deg, sr = case_signals(sfx, efx, name)
        st = E.estoi_stages(ref, deg, sr)
        d[name], M[name] = st['d'], st['M']
        r = st['ratios']
        assert E.margin_ok(r), (name, r[(r >= E.MARGIN[0]) & (r <= E.MARGIN[1])])
        kept, dropped = r[r > E.ZERO_RULE], r[r <= E.ZERO_RULE]
        ratio_gap[name] = (float(kept.min()) if kept.size else math.inf,
                           float(dropped.max()) if dropped.size else 0.0)
        if name in DM_CASES:
            dm[name] = torch.from_numpy(st['dm'].copy())
        if name == 'zero_run':
            assert st['zeroed'] > 0 and dropped.size > 0
            efx['zero_run'] = {'zeroed': st['zeroed'], 'dropped_with_energy': int(dropped.size),
                               'smallest_kept': ratio_gap[name][0],
                               'largest_dropped': ratio_gap[name][1]}
    for name, m in SLICES:
        assert M[name] == m, (name, M[name])
    assert math.isnan(d['m30']) and dm['m31'].numel() == 1 and dm['m32'].numel() == 2
    assert math.isnan(d['short']) and math.isnan(d['silent'])
    assert all(math.isfinite(v) for k, v in d.items() if k not in ('short', 'silent', 'm30')), d
    snr_d = [d['snr{}'.format(s).replace('-', 'm')] for s in G.SNRS]
    assert all(a < b for a, b in zip(snr_d, snr_d[1:])), snr_d
    assert abs(d['scaled'] - 1) < 1e-12, d['scaled']

    cli = sfx['cli']
    cd = []
    for c, n in zip(cli['clean'], cli['noisy']):
        L = min(c.numel(), n.numel())
        cd.append(E.estoi(G.to_float(c.numpy())[:L], G.to_float(n.numpy())[:L], G.SR))
    assert all(math.isfinite(v) for v in cd), cd

    efx.update(d=d, dm=dm, M=M, ratio_gap=ratio_gap, cli_d=torch.tensor(cd, dtype=torch.float64),
               meta={'recipe': 'scripts/make_golden_estoi.py', 'oracle': 'scripts/estoi_oracle.py',
                     'signals': 'tests/golden/stoi.pt', 'numpy': np.__version__})
    torch.save(efx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')
    for k in names:
        print('  {:9s} d = {:.12f}  M = {:3d}  e/raw kept >= {:.3g}, dropped <= {:.3g}'.format(
            k, d[k], M[k], *ratio_gap[k]))
    print('  slices', {n: rc['len'] for n, rc in efx['extra_cases'].items()})
    print('  zero_run', efx['zero_run'])
    print('  cli', ['{:.4f}'.format(v) for v in cd])


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'estoi.pt'))
