"""Writes tests/golden/denoise.pt: the fixture of ops.denoise_rows / ops.denoise_stages and
baselines.wiener / logmmse, computed with the numpy oracle scripts/denoise_oracle.py (DESIGN.md
section 20).

    python scripts/make_golden_denoise.py [out.pt]

Everything is synthetic (seeded numpy) and stored as float32, so that no sine of another machine's
libm enters a test:

  signals   clean (a gated harmonic signal, 32000 samples at 16 kHz: 200 ms of silence, then three
            voiced stretches), noisy (clean + white noise at 5 dB over the voiced stretches),
            clean8 / noisy8 (the like at 8 kHz, 8000 samples)
  cases     name -> {'nframes', 'vad' (v_t), 'update' (the noise-update flag of every frame),
            'margin' (|v_t - 0.15|)} per rule, and 'y' for the rows of at most Y_UP_TO samples;
            the rows themselves are made by `case_rows` from the signals
  meta      what the tolerances of the GPU tests rest on: for each rule and quantity the largest
            movement of the oracle between float64 and numpy.longdouble over all cases (y relative
            to max |x| of the row, v_t relative to max(1, |v_t|)), and the smallest decision margin
            of any frame

It asserts that no frame of any case has |v_t - 0.15| below 1e-7 (and moves on to the next seed if
one does), and that float64 and longdouble agree on every noise-update flag.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import denoise_oracle as O  # noqa: E402

SEED = 20262
MARGIN = 1e-7
N = 32000
N8 = 8000
LENGTHS = (1919, 1920, 2079, 2080, 8000, 32000)
Y_UP_TO = 2080               # y is stored for the rows of at most this many samples
SNR_DB = 5.0


def gated(n, srate, f0=150.0, amp=0.1):
    """(signal, active): silence to 200 ms, then voiced stretches of eight harmonics with short
    silences between them; digital zeros in the silences."""
    t = np.arange(n) / float(srate)
    sig = np.zeros(n)
    for h in range(1, 9):
        if h * f0 * 1.1 < srate / 2:
            sig += np.sin(2 * np.pi * h * f0 * (1 + 0.05 * np.sin(2 * np.pi * 2 * t)) * t + h) / h
    active = np.zeros(n, bool)
    for a, b in ((0.2, 0.45), (0.6, 1.1), (1.3, 1.8)):
        active |= (t >= a) & (t < b)
    return amp * sig * active, active


def add_noise(sig, active, snr_db, rng):
    """sig + white noise with `snr_db` over the active samples."""
    nz = rng.standard_normal(len(sig))
    g = np.sqrt(np.mean(sig[active] ** 2) / np.mean(nz[active] ** 2) / 10.0 ** (snr_db / 10.0))
    return sig + g * nz


def active_snr(clean, y, active, upto=None):
    """SNR in dB of y against clean over the active samples below `upto`."""
    m = active.copy()
    if upto is not None:
        m[upto:] = False
    c = clean.astype(np.float64)[m]
    e = np.asarray(y, np.float64)[m] - c
    return 10.0 * np.log10(np.sum(c * c) / np.sum(e * e))


def make_signals(seed):
    rng = np.random.default_rng(seed)
    c, a = gated(N, 16000)
    c8, a8 = gated(N8, 8000)
    sig = {'clean': c, 'noisy': add_noise(c, a, SNR_DB, rng),
           'clean8': c8, 'noisy8': add_noise(c8, a8, SNR_DB, rng)}
    return {k: v.astype(np.float32) for k, v in sig.items()}


def case_rows(signals):
    """name -> (row float32, srate): every case of the GPU test."""
    x = np.asarray(signals['noisy'], np.float32)
    rows = {'L{}'.format(L): (x[:L].copy(), 16000) for L in LENGTHS}
    rows['rate8'] = (np.asarray(signals['noisy8'], np.float32).copy(), 8000)
    rows['zero'] = (np.zeros(8000, np.float32), 16000)
    s = x[:8000].copy()
    s[:3000] = 0
    rows['silent_start'] = (s, 16000)
    rows['scaled'] = (x[:8000] * np.float32(2.0 ** -10), 16000)
    return rows


def gap(a, b, x):
    """The movement between two runs of the oracle (float64, longdouble) on the row x."""
    assert a['nframes'] == b['nframes'] and np.array_equal(a['update'], b['update'])
    peak = float(np.max(np.abs(x))) if len(x) else 0.0
    dy = float(np.max(np.abs(np.asarray(a['y'] - b['y'], np.float64)))) if len(x) else 0.0
    assert peak > 0 or dy == 0
    g = {'y': dy / peak if peak > 0 else 0.0, 'vad': 0.0}
    if a['nframes']:
        dv = np.abs(np.asarray(a['vad'] - b['vad'], np.float64))
        g['vad'] = float(np.max(dv / np.maximum(1.0, np.abs(a['vad']))))
    return g


def build(seed):
    """The fixture for `seed`, or None where a frame's decision margin is below MARGIN."""
    import torch
    signals = make_signals(seed)
    gaps = {rule: {'y': 0.0, 'vad': 0.0} for rule in O.RULES}
    cases, margins = {}, []
    for name, (x, srate) in case_rows(signals).items():
        cases[name] = {}
        for rule in O.RULES:
            a = O.denoise(x, srate, rule)
            b = O.denoise(x, srate, rule, dtype=np.longdouble)
            for k, v in gap(a, b, x).items():
                gaps[rule][k] = max(gaps[rule][k], v)
            margins.append(a['margin'])
            c = {'nframes': a['nframes'], 'vad': torch.from_numpy(a['vad'].copy()),
                 'update': torch.from_numpy(a['update'].copy()),
                 'margin': torch.from_numpy(a['margin'].copy())}
            if len(x) <= Y_UP_TO:
                c['y'] = torch.from_numpy(a['y'].copy())
            cases[name][rule] = c
    margin = float(min(m.min() for m in margins if len(m)))
    if margin < MARGIN:
        return None
    return {'signals': {k: torch.from_numpy(v) for k, v in signals.items()}, 'cases': cases,
            'lengths': list(LENGTHS),
            'meta': {'recipe': 'scripts/make_golden_denoise.py',
                     'oracle': 'scripts/denoise_oracle.py', 'seed': seed, 'gaps': gaps,
                     'min_margin': margin, 'margin_floor': MARGIN, 'snr_db': SNR_DB,
                     'frames': int(sum(len(m) for m in margins)), 'numpy': np.__version__}}


def main(out):
    import torch
    for seed in range(SEED, SEED + 20):
        fx = build(seed)
        if fx is not None:
            break
        print('seed', seed, 'has a frame with a decision margin below', MARGIN)
    else:
        raise SystemExit('no seed without a close decision')
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes; seed', fx['meta']['seed'])
    print('  frames', fx['meta']['frames'], ' smallest margin', fx['meta']['min_margin'])
    print('  gaps', fx['meta']['gaps'])
    for name, c in fx['cases'].items():
        print('  {:13s}'.format(name), {r: (v['nframes'], int(v['update'].sum()))
                                        for r, v in c.items()})


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'denoise.pt'))
