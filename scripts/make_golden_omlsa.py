"""Writes tests/golden/omlsa.pt: the fixture of ops.omlsa_rows / ops.omlsa_stages and
baselines.omlsa, computed with the numpy oracle scripts/omlsa_oracle.py.

    python scripts/make_golden_omlsa.py [out.pt]

Everything is synthetic (seeded numpy) and stored as float32, as in scripts/make_golden_denoise.py,
whose gated signal and noise mixing are used here:

  signals   noisy (32000 samples at 16 kHz) and noisy8 (8000 samples at 8 kHz) as in denoise.pt,
            from this recipe's own seed; clean4 (64000 samples at 16 kHz: six voiced stretches) and
            noise4 (white noise of the same length)
  gains     the noise gain that puts noise4 5 dB below the voiced samples of clean4 after 2.5 s,
            and that gain 10 dB lower and 10 dB higher.  The four long rows flat, step_up,
            step_down and ramp are clean4 + gain[n] noise4 in float32 arithmetic (`long_rows`): the
            late gain throughout; the low gain before 1.0 s; the high gain before 1.0 s; a gain
            rising linearly by 10 dB over the first 3 s (between two gains of its own, so that its
            noise is at 5 dB after 2.5 s as well).  The rows are not stored: four rows of 64000
            samples would not fit a committed file
  cases     name -> {'nframes', 'presence', 'rough', 'noise', 'margin'} and 'y' for the rows of at
            most Y_UP_TO samples; the rows themselves are made by `case_rows` from the signals
  meta      what the tolerances of the GPU tests rest on: the largest movement of the oracle between
            float64 and numpy.longdouble over all cases (y relative to max |x| of the row, presence
            absolute, noise relative to its own maximum), the smallest margin of the discontinuous
            comparisons, and for the four long rows the SNR over the voiced samples after 2.5 s of
            the noisy row and of the three oracles (wiener, logmmse, omlsa)

A seed is refused (and the next one tried) where a case's margin is below MARGIN.  float64 and
longdouble have to agree on every rough count.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import denoise_oracle as D  # noqa: E402
import make_golden_denoise as GD  # noqa: E402
import omlsa_oracle as O  # noqa: E402

SEED = 20263
MARGIN = 1e-9
N4 = 64000
LENGTHS = (1919, 1920, 2079, 2080, 8000, 32000)
Y_UP_TO = 2080               # y is stored for the rows of at most this many samples
SNR_DB = 5.0
CHANGE_DB = 10.0
LATE = 2.5                   # seconds: the SNR of the long rows is taken from here on
LONG = ('flat', 'step_up', 'step_down', 'ramp')
# the ramp's position between its two gains: 0 .. 1 over the first 3 s, float32
RAMP_FRAC = np.minimum(np.arange(N4), 48000).astype(np.float32) / np.float32(48000)
STRETCHES = ((0.2, 0.45), (0.6, 1.1), (1.3, 1.8), (2.0, 2.4), (2.6, 3.1), (3.3, 3.8))


def gated6(n=N4, srate=16000, f0=150.0, amp=0.1):
    """(signal, active): GD.gated's harmonic signal with six voiced stretches over four seconds."""
    t = np.arange(n) / float(srate)
    sig = np.zeros(n)
    for h in range(1, 9):
        if h * f0 * 1.1 < srate / 2:
            sig += np.sin(2 * np.pi * h * f0 * (1 + 0.05 * np.sin(2 * np.pi * 2 * t)) * t + h) / h
    active = np.zeros(n, bool)
    for a, b in STRETCHES:
        active |= (t >= a) & (t < b)
    return amp * sig * active, active


def late_mask(active, srate=16000):
    m = active.copy()
    m[:int(LATE * srate)] = False
    return m


def late_snr(clean, y, active, srate=16000):
    """SNR in dB of y against clean over the voiced samples after 2.5 s."""
    m = late_mask(active, srate)
    c = np.asarray(clean, np.float64)[m]
    e = np.asarray(y, np.float64)[m] - c
    return 10.0 * np.log10(np.sum(c * c) / np.sum(e * e))


def make_signals(seed):
    """(signals, gains): float32 arrays, and the noise gains as the float32 values the long rows
    are built with: late, low, high, and the ramp's own two ends (the ramp still rises after
    2.5 s, so its late gain is a little above the others')."""
    rng = np.random.default_rng(seed)
    c, a = GD.gated(GD.N, 16000)
    c8, a8 = GD.gated(GD.N8, 8000)
    sig = {'noisy': GD.add_noise(c, a, SNR_DB, rng), 'noisy8': GD.add_noise(c8, a8, SNR_DB, rng)}
    c4, a4 = gated6()
    sig['clean4'], sig['noise4'] = c4, rng.standard_normal(N4)
    sig = {k: v.astype(np.float32) for k, v in sig.items()}
    late = late_mask(a4)
    c4, nz = sig['clean4'].astype(np.float64), sig['noise4'].astype(np.float64)
    step = 10.0 ** (CHANGE_DB / 20.0)

    def gain(shape):         # the gain g with which c4 + g shape nz has SNR_DB over `late`
        return np.sqrt(np.mean(c4[late] ** 2) / np.mean((shape * nz)[late] ** 2) /
                       10.0 ** (SNR_DB / 10.0))

    g, gr = gain(1.0), gain(1.0 / step + (1.0 - 1.0 / step) * RAMP_FRAC.astype(np.float64))
    gains = {'late': g, 'low': g / step, 'high': g * step, 'ramp_low': gr / step, 'ramp_late': gr}
    return sig, {k: float(np.float32(v)) for k, v in gains.items()}


def long_rows(signals, gains):
    """kind -> row float32: clean4 + gain[n] noise4 in float32 arithmetic, the gain being the late
    one throughout (flat), the low or the high one before 1.0 s (step_up, step_down), or rising
    linearly from the low to the late one over the first 3 s (ramp)."""
    c4 = np.asarray(signals['clean4'], np.float32)
    nz = np.asarray(signals['noise4'], np.float32)
    late, low, high, rlow, rlate = (np.float32(gains[k]) for k in (
        'late', 'low', 'high', 'ramp_low', 'ramp_late'))
    n = np.arange(N4)
    gain = {'flat': np.full(N4, late, np.float32),
            'step_up': np.where(n < 16000, low, late).astype(np.float32),
            'step_down': np.where(n < 16000, high, late).astype(np.float32),
            'ramp': rlow + (rlate - rlow) * RAMP_FRAC}
    return {kind: c4 + gain[kind] * nz for kind in LONG}


def case_rows(signals, gains):
    """name -> (row float32, srate): every case of the GPU test."""
    rows = GD.case_rows(signals)
    for kind, x in long_rows(signals, gains).items():
        assert x.dtype == np.float32
        rows[kind] = (x, 16000)
    return rows


def gap(a, b, x):
    """The movement between two runs of the oracle (float64, longdouble) on the row x."""
    assert a['nframes'] == b['nframes'] and np.array_equal(a['rough'], b['rough'])
    peak = float(np.max(np.abs(x))) if len(x) else 0.0
    dy = float(np.max(np.abs(np.asarray(a['y'] - b['y'], np.float64)))) if len(x) else 0.0
    assert peak > 0 or dy == 0
    g = {'y': dy / peak if peak > 0 else 0.0, 'presence': 0.0, 'noise': 0.0}
    if a['nframes']:
        g['presence'] = float(np.max(np.abs(np.asarray(a['presence'] - b['presence'], np.float64))))
        top = float(np.max(a['noise']))
        g['noise'] = float(np.max(np.abs(np.asarray(a['noise'] - b['noise'], np.float64)))) / top
    return g


def late_snrs(signals, gains):
    """kind -> {'noisy', 'wiener', 'logmmse', 'omlsa'}: the late-voiced SNR of the oracles."""
    clean = np.asarray(signals['clean4'], np.float64)
    _, active = gated6()
    out = {}
    for kind, x in long_rows(signals, gains).items():
        out[kind] = {'noisy': late_snr(clean, x, active),
                     'wiener': late_snr(clean, D.wiener(x), active),
                     'logmmse': late_snr(clean, D.logmmse(x), active),
                     'omlsa': late_snr(clean, O.omlsa(x)['y'], active)}
    return out


def build(seed, snrs=True):
    """The fixture for `seed`, or None where a case's margin is below MARGIN."""
    import torch
    signals, gains = make_signals(seed)
    gaps = {'y': 0.0, 'presence': 0.0, 'noise': 0.0}
    cases, margins = {}, []
    for name, (x, srate) in case_rows(signals, gains).items():
        a = O.omlsa(x, srate)
        if a['margin'] < MARGIN:
            return None
        b = O.omlsa(x, srate, dtype=np.longdouble)
        for k, v in gap(a, b, x).items():
            gaps[k] = max(gaps[k], v)
        margins.append(a['margin'])
        c = {'nframes': a['nframes'], 'presence': torch.from_numpy(a['presence'].copy()),
             'rough': torch.from_numpy(a['rough'].copy()),
             'noise': torch.from_numpy(a['noise'].copy()), 'margin': a['margin']}
        if len(x) <= Y_UP_TO:
            c['y'] = torch.from_numpy(a['y'].copy())
        cases[name] = c
    meta = {'recipe': 'scripts/make_golden_omlsa.py', 'oracle': 'scripts/omlsa_oracle.py',
            'seed': seed, 'gaps': gaps, 'min_margin': float(min(margins)), 'margin_floor': MARGIN,
            'snr_db': SNR_DB, 'change_db': CHANGE_DB, 'late': LATE, 'numpy': np.__version__}
    if snrs:
        meta['late_snr'] = late_snrs(signals, gains)
    return {'signals': {k: torch.from_numpy(v) for k, v in signals.items()}, 'gains': gains,
            'cases': cases, 'lengths': list(LENGTHS), 'meta': meta}


def main(out):
    import torch
    for seed in range(SEED, SEED + 20):
        fx = build(seed)
        if fx is not None:
            break
        print('seed', seed, 'has a comparison with a margin below', MARGIN)
    else:
        raise SystemExit('no seed without a close decision')
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes; seed', fx['meta']['seed'])
    print('  smallest margin', fx['meta']['min_margin'])
    print('  gaps', fx['meta']['gaps'])
    for kind, v in fx['meta']['late_snr'].items():
        print('  {:10s}'.format(kind), {k: round(s, 2) for k, s in v.items()})
    for name, c in fx['cases'].items():
        print('  {:13s}'.format(name), c['nframes'], int(c['rough'].sum()), c['margin'])


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'omlsa.pt'))
