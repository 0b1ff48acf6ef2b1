"""Writes tests/golden/pyin.pt: the fixture of ops.pyin / ops.pyin_stages and of tracker='pyin' in
quality.pitch / quality.f0_eval, computed with the numpy oracle scripts/pyin_oracle.py (DESIGN.md
section 22).

    python scripts/make_golden_pyin.py [out.pt]

Everything is synthetic (seeded numpy) and stored as float32:

  signals   tone (a harmonic glide 110 -> 150 Hz at 10 dB SNR, 8000 samples), tone8 (the like at
            8 kHz, 4000 samples), gated5 (silence, voiced, unvoiced, voiced, silence, voiced, every
            voiced stretch at the centre of one pitch bin, in white noise at 5 dB SNR, 12000
            samples), octave (100 Hz, a glide to 200 Hz in 0.3 s, 200 Hz, at 15 dB SNR; 8000 samples)
  rows      for every row of `rows()` (the prefixes of tone where the framing can go wrong, the
            zero row, the row that starts in 3000 zeros, tone times 2^-10 and the signals above) the
            oracle's contour with its own tables: f0, lag, vprob, state, the last frame's delta;
            `gap`, the smallest relative gap between winner and runner-up over the decisions on the
            decoded path, exact ties excluded; `move`, the largest movement of f0, vprob, bv and
            delta (relative to the value; bv and delta to the frame's largest) between float64 and
            numpy.longdouble

A row whose float64 and long-double paths (state and lag on every frame) differ is refused: the seed
moves on.  Such rows exist: while the path is unvoiced every bin has the same observation, so two
orders of the same bin steps through an unvoiced stretch tie up to rounding.  That is why gated5
keeps one pitch bin: a gap with the same bin on both sides is crossed without a step.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_pitch as GP  # noqa: E402
import pyin_oracle as Y  # noqa: E402

SEED = 20270
N, N8, NG = 8000, 4000, 12000
PREFIXES = (666, 667, 747, 1707, 8000)
GATED_BIN = 62                   # 123.5 Hz


def gated_flat(n, srate, f, rng):
    """silence, voiced, unvoiced, voiced, silence, voiced, all voiced stretches at f Hz"""
    cut = [int(round(c * n)) for c in (0.0, 0.09, 0.37, 0.49, 0.79, 0.885, 1.0)]
    x = np.zeros(n)
    for (a, b), kind in zip(zip(cut[:-1], cut[1:]), (None, 'v', 'noise', 'v', None, 'v')):
        m = b - a
        if kind is None:
            continue
        if kind == 'noise':
            seg = 0.05 * rng.standard_normal(m)
        else:
            seg = 0.3 * GP.harmonics(np.full(m, f), srate)
        x[a:b] = seg * GP._fade(m, srate)
    return x


def make_signals(seed):
    rng = np.random.default_rng(seed)

    def noisy(x, snr):
        return x + 10 ** (-snr / 20) * np.sqrt(np.mean(x ** 2)) * rng.standard_normal(len(x))

    f = Y.FMIN * 2.0 ** ((GATED_BIN + 0.5) / Y.BINS_PER_OCTAVE)
    ramp = np.concatenate([np.full(1600, 100.0), np.geomspace(100, 200, 4800), np.full(1600, 200.0)])
    sig = {'tone': noisy(0.3 * GP.harmonics(np.geomspace(110, 150, N), 16000), 10),
           'tone8': noisy(0.3 * GP.harmonics(np.geomspace(100, 130, N8), 8000), 10),
           'gated5': noisy(gated_flat(NG, 16000, f, rng), 5),
           'octave': noisy(0.3 * GP.harmonics(ramp, 16000), 15)}
    return {k: v.astype(np.float32) for k, v in sig.items()}


def rows(signals):
    """name -> (row, srate) of every row the tests run, from the fixture's signals (numpy)"""
    tone = signals['tone']
    out = {'tone[:{}]'.format(L): (tone[:L], 16000) for L in PREFIXES}
    out['tone8'] = (signals['tone8'], 8000)
    out['zero'] = (np.zeros(2000, np.float32), 16000)
    out['lead'] = (np.concatenate([np.zeros(3000, np.float32), tone[:5000]]), 16000)
    out['tone*2^-10'] = (tone * np.float32(2.0 ** -10), 16000)
    out['gated5'] = (signals['gated5'], 16000)
    out['octave'] = (signals['octave'], 16000)
    return out


def movement(a, b):
    """the largest movement between two runs of the oracle of one row (same path)"""
    def rel(x, y, scale):
        x, y = np.asarray(x, np.longdouble), np.asarray(y, np.longdouble)
        s = np.asarray(scale, np.longdouble)
        ok = s > 0
        assert not (x - y)[~ok].any()
        return float(np.max(np.abs(x - y)[ok] / s[ok])) if ok.any() else 0.0

    nf = len(a['lag'])
    if nf == 0:
        return {'f0': 0.0, 'vprob': 0.0, 'bv': 0.0, 'delta': 0.0}
    top = np.maximum(a['bv'].max(axis=1, keepdims=True), 0) * np.ones_like(a['bv'])
    return {'f0': rel(a['f0'], b['f0'], a['f0']), 'vprob': rel(a['vprob'], b['vprob'], a['vprob']),
            'bv': rel(a['bv'], b['bv'], top),
            'delta': rel(a['delta'], b['delta'], np.full(len(a['delta']), a['delta'].max()))}


def build(seed):
    """The fixture for `seed`, or the name of a row whose float64 and long-double paths differ."""
    import torch
    signals = make_signals(seed)
    packed = {}
    for name, (x, srate) in rows(signals).items():
        a = Y.track(x, srate)
        b = Y.track(x, srate, dtype=np.longdouble)
        if not (np.array_equal(a['state'], b['state']) and np.array_equal(a['lag'], b['lag'])):
            return name
        packed[name] = {'f0': torch.from_numpy(a['f0']), 'lag': torch.from_numpy(a['lag']),
                        'vprob': torch.from_numpy(a['vprob']),
                        'state': torch.from_numpy(a['state']),
                        'delta': torch.from_numpy(a['delta']), 'gap': float(a['gap']),
                        'move': movement(a, b), 'srate': srate}
    return {'signals': {k: torch.from_numpy(v) for k, v in signals.items()}, 'rows': packed,
            'meta': {'recipe': 'scripts/make_golden_pyin.py', 'oracle': 'scripts/pyin_oracle.py',
                     'seed': seed, 'numpy': np.__version__}}


def main(out):
    import torch
    for seed in range(SEED, SEED + 40):
        fx = build(seed)
        if not isinstance(fx, str):
            break
        print('seed', seed, 'refused: float64 and long double decode', fx, 'differently')
    else:
        raise SystemExit('no seed whose rows all decode alike in both precisions')
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes; seed', fx['meta']['seed'])
    for name, r in fx['rows'].items():
        print('  {:12s} frames {:4d} voiced {:4d} gap {:.3g} move {}'.format(
            name, len(r['lag']), int((r['lag'] > 0).sum()), r['gap'],
            {k: float('{:.3g}'.format(v)) for k, v in r['move'].items()}))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'pyin.pt'))
