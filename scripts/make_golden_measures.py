"""Writes tests/golden/measures.pt: the fixture of ops.fwsegsnr / ops.cepstral_distance /
ops.si_sdr and their quality.* wrappers, computed with the fp64 numpy oracle
scripts/measures_oracle.py.

    python scripts/make_golden_measures.py [out.pt]

The fixture stores no signals: every case names a track, a noise track and a gain of
tests/golden/quality.pt by key, and a slice of them (`CASES`); `case_signals(qfx, name)` rebuilds
the pair the way quality.pt's own recipe does (clean + float32(gain) * noise in float32).  Stored:
the per-frame fwSNRseg and CD, their utterance values and the SI-SDR of every case, the three
measures of quality.pt's eval-CLI wav pairs, and in `meta` what the tolerances of the GPU tests
rest on:

  * cd_sensitivity_max: the largest per-frame change of the oracle's own CD when its lag sums run
    in reversed order, or everything runs in numpy.longdouble.  The GPU tolerance is
    max(100 x that, 1e-9); the recipe asserts it stays within LLR's 1e-4.
  * sisdr_moments_gap: the largest |si_sdr - si_sdr_moments| in dB (alpha and the means from the
    one-pass moments, as the kernel takes them), asserted to be below 1e-9.

It asserts too that every band of every finite fwSNRseg frame has |ce - pe| >= 1e-6 ce (the
cancellation in err cannot lift rounding past the 1e-6 tolerance) and that no unclipped frame lies
within 1e-6 of -10 or 35 (a clip decision cannot flip).
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import measures_oracle as M  # noqa: E402

ZERO_RUN = (20000, 22000)     # quality.pt's zero_run recipe: exact zeros in the clean signal
CASES = {
    'snr0': dict(ref='clean', noise='noise', gain='snr0', start=0, len=40000, srate=16000),
    'snr10': dict(ref='clean', noise='noise', gain='snr10', start=0, len=40000, srate=16000),
    'snr20': dict(ref='clean', noise='noise', gain='snr20', start=0, len=40000, srate=16000),
    'slice': dict(ref='clean', noise='noise', gain='snr10', start=8000, len=12345, srate=16000),
    'zero_run': dict(ref='clean', noise='noise', gain='snr10', start=0, len=40000, srate=16000,
                     zero_ref=ZERO_RUN),
    'sr8k': dict(ref='clean8', noise='noise8', gain='sr8k', start=0, len=16000, srate=8000),
}
CD_LIMIT = 1e-4               # LLR's tolerance: 100 x the sensitivity must stay within it
CD_FLOOR = 1e-9


def case_signals(qfx, name, cases=CASES):
    """(ref, deg, srate) of case `name`, float32, from quality.pt's signals and gains."""
    rc = cases[name]
    clean = qfx['signals'][rc['ref']].numpy()
    noise = qfx['signals'][rc['noise']].numpy()
    deg = (clean + np.float32(qfx['gains'][rc['gain']]) * noise).astype(np.float32)
    ref = clean.copy()
    if 'zero_ref' in rc:
        a, b = rc['zero_ref']
        ref[a:b] = 0
    sl = slice(rc['start'], rc['start'] + rc['len'])
    return ref[sl], deg[sl], rc['srate']


def cli_signals(qfx):
    """quality.pt's three eval-CLI pairs as the CLI reads them: int16 / 32768, common length."""
    out = []
    for c, n in zip(qfx['cli']['clean'], qfx['cli']['noisy']):
        L = min(c.numel(), n.numel())
        out.append((c.numpy()[:L].astype(np.float32) / 32768,
                    n.numpy()[:L].astype(np.float32) / 32768))
    return out


def cd_tolerance(meta):
    return max(100.0 * meta['cd_sensitivity_max'], CD_FLOOR)


def evaluate(ref, deg, srate):
    fw = M.fwsegsnr_frames(ref, deg, srate)
    cd = M.cd_frames(ref, deg, srate)
    return {'fw_frames': fw, 'fw': M.finite_mean(fw), 'cd_frames': cd, 'cd': M.trimmed_mean(cd),
            'sisdr': M.si_sdr(ref, deg)}


def check_margins(name, ref, deg, srate):
    ce, pe = M.fwsegsnr_bands(ref, deg, srate)
    raw = M.fwsegsnr_frames(ref, deg, srate, clip=False)
    fin = np.isfinite(raw)
    assert np.all(np.abs(ce[fin] - pe[fin]) >= 1e-6 * ce[fin]), name
    assert not np.any(np.abs(raw[fin] + 10.0) <= 1e-6) and not np.any(np.abs(raw[fin] - 35.0) <= 1e-6), name
    return int(fin.sum()), float(np.min(np.abs(ce[fin] - pe[fin]) / ce[fin]))


def cd_sensitivity(ref, deg, srate):
    base = M.cd_frames(ref, deg, srate)
    worst = 0.0
    for other in (M.cd_frames(ref, deg, srate, order='reversed'),
                  M.cd_frames(ref, deg, srate, dtype=np.longdouble)):
        assert np.array_equal(np.isnan(base), np.isnan(other))
        fin = np.isfinite(base)
        if fin.any():
            worst = max(worst, float(np.abs(base[fin] - other[fin]).max()))
    return worst


def main(out):
    import torch
    qfx = torch.load(os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'quality.pt'),
                     map_location='cpu', weights_only=False)
    results, sens, gap, margins = {}, 0.0, 0.0, {}
    for name in CASES:
        ref, deg, sr = case_signals(qfx, name)
        r = evaluate(ref, deg, sr)
        margins[name] = check_margins(name, ref, deg, sr)
        sens = max(sens, cd_sensitivity(ref, deg, sr))
        gap = max(gap, abs(r['sisdr'] - M.si_sdr_moments(ref, deg)))
        assert r['fw_frames'].shape == r['cd_frames'].shape == (M.frame_count(len(ref), sr),)
        assert np.array_equal(np.isnan(r['fw_frames']), np.isnan(r['cd_frames'])), name
        assert all(math.isfinite(r[k]) for k in ('fw', 'cd', 'sisdr')), (name, r)
        results[name] = {k: (torch.from_numpy(v.copy()) if isinstance(v, np.ndarray) else v)
                         for k, v in r.items()}
    nan_frames = int(np.isnan(results['zero_run']['fw_frames'].numpy()).sum())
    assert nan_frames > 0 and all(
        not np.isnan(results[n]['fw_frames'].numpy()).any() for n in CASES if n != 'zero_run')
    for k, up in (('fw', True), ('sisdr', True), ('cd', False)):
        v = [results[n][k] for n in ('snr0', 'snr10', 'snr20')]
        assert all((a < b) == up for a, b in zip(v, v[1:])), (k, v)
    assert 100.0 * sens <= CD_LIMIT, sens
    assert gap < 1e-9, gap

    cli = [evaluate(c, n, 16000) for c, n in cli_signals(qfx)]
    fx = {'cases': CASES, 'results': results,
          'cli': {k: torch.tensor([r[k] for r in cli], dtype=torch.float64)
                  for k in ('fw', 'cd', 'sisdr')},
          'meta': {'recipe': 'scripts/make_golden_measures.py',
                   'oracle': 'scripts/measures_oracle.py', 'signals': 'tests/golden/quality.pt',
                   'cd_sensitivity_max': sens, 'sisdr_moments_gap': gap,
                   'zero_run_nan_frames': nan_frames, 'numpy': np.__version__}}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')
    for n in CASES:
        r = results[n]
        print('  {:9s} fwSNRseg = {:.9f}  CD = {:.9f}  SI-SDR = {:.9f}  finite frames {}, '
              'min |ce-pe|/ce = {:.3g}'.format(n, r['fw'], r['cd'], r['sisdr'], *margins[n]))
    print('  cd_sensitivity_max', sens, '-> tolerance', cd_tolerance(fx['meta']))
    print('  sisdr_moments_gap', gap, ' zero_run NaN frames', nan_frames)
    print('  cli', {k: ['{:.4f}'.format(v) for v in t.tolist()] for k, t in fx['cli'].items()})


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'measures.pt'))
