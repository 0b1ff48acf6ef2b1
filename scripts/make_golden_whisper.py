"""Writes tests/golden/whisper.pt: the fixture of the whisper stage (ops.whisper_rows /
whisper_stages, augment.Whisper), computed by the float64 numpy oracle
scripts/whisper_oracle.py.

    python scripts/make_golden_whisper.py [out.pt]

Every row is a periodic test signal made here (`whisper_oracle.voiced`: an impulse train at f0 plus
1 % white noise through three two-pole resonances at 700 / 1200 / 2600 Hz under a slow Hann-shaped
envelope, quantised to int16 steps), at most 4096 samples long, with zeros written into it where a
case asks for silence.

Per case the oracle runs twice, in float64 and in np.longdouble.  `move` records how far each
result moves between the two, relative to the largest magnitude of that result: the oracle's own
rounding error, which the GPU tests multiply by 100 for their tolerance (the SRMR precedent).  A
case whose output moves by more than 1e-10 of max |y| is refused as ill-conditioned, and so is one
whose status, silent frames or orders differ between the two precisions.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import whisper_oracle as W  # noqa: E402

MAX_MOVE = 1e-10

# T = 1, 77, 255, 256, 257, 1500, 4096; len < T; len = 0 with and without prev; len a multiple of
# the hop; silence of more than two frames inside a row; an all-zero row; tilt 0 and 0.9; prev zero
# and not; a row whose whispered peak exceeds 1; another lag window
CASES = {
    'one': dict(T=1, f0=180, seed=11, tilt=0.0, prev=0.3),
    'short': dict(T=77, f0=180, seed=12, tilt=0.9, prev=-0.2),
    't255': dict(T=255, f0=240, seed=13, tilt=0.5, prev=0.0),
    't256': dict(T=256, f0=240, seed=14, tilt=0.0, prev=0.05),
    't257': dict(T=257, f0=240, seed=15, tilt=0.9, prev=0.0),
    'odd': dict(T=1500, f0=110, seed=16, tilt=0.5, prev=0.1),
    'full': dict(T=4096, f0=110, seed=17, tilt=0.0, prev=0.0),
    'full_tilt': dict(T=4096, f0=240, seed=2 ** 63 - 1, tilt=0.9, prev=-0.01),
    'partial': dict(T=1500, f0=180, seed=18, tilt=0.0, prev=0.02, length=1000),
    'len_hop': dict(T=1500, f0=180, seed=19, tilt=0.9, prev=0.0, length=1024),
    'empty_prev': dict(T=77, f0=180, seed=20, tilt=0.5, prev=0.25, length=0),
    'empty': dict(T=77, f0=180, seed=21, tilt=0.5, prev=0.0, length=0),
    'gap': dict(T=4096, f0=180, seed=0, tilt=0.5, prev=0.0, zero=(1000, 2400)),
    'zeros': dict(T=300, f0=180, seed=23, tilt=0.0, prev=0.0, zero=(0, 300)),
    'guard': dict(T=4096, f0=180, seed=5, tilt=0.0, prev=0.0, peak=0.9, sig_seed=1),
    'lag60': dict(T=1500, f0=110, seed=24, tilt=0.0, prev=0.1, lag_hz=60.0),
}


def signal(c):
    x = W.voiced(c['f0'], c['T'], c.get('sig_seed', c['seed'] % 1000), peak=c.get('peak', 0.5))
    if 'zero' in c:
        x[c['zero'][0]:c['zero'][1]] = 0
    return x


def rel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    m = np.abs(b).max() if b.size else 0
    return float(np.abs(a - b).max() / m) if m > 0 else 0.0


def make_case(name, c):
    x = signal(c)
    kw = dict(length=c.get('length'), prev=c['prev'], lag_hz=c.get('lag_hz', 120.0))
    o = W.whisper(x, c['seed'], c['tilt'], dtype=np.float64, **kw)
    ol = W.whisper(x, c['seed'], c['tilt'], dtype=np.longdouble, **kw)
    for k in ('status', 'nsilent', 'minorder'):
        assert o[k] == ol[k], (name, k, o[k], ol[k])
    assert (o['order'] == ol['order']).all(), (name, o['order'], ol['order'])
    move = {k: rel(o[k], ol[k]) for k in ('r', 'a', 'sigma', 'y')}
    move['peak'] = rel(o['peak'], ol['peak'])
    assert move['y'] <= MAX_MOVE, '{}: ill-conditioned, y moves by {}'.format(name, move['y'])
    t = lambda v, dt=torch.float64: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dt)  # noqa: E731
    return dict(x=torch.from_numpy(x), seed=int(c['seed']), tilt=float(c['tilt']),
                length=c.get('length'), prev=float(np.float32(c['prev'])), lag_hz=kw['lag_hz'],
                r=t(o['r']), a=t(o['a']), sigma=t(o['sigma']), order=t(o['order'], torch.int32),
                y=t(o['y']), out=t(o['out']), prev_out=float(o['prev_out']), peak=float(o['peak']),
                status=int(o['status']), nsilent=int(o['nsilent']), minorder=int(o['minorder']),
                move=move)


def main(out):
    cases = {name: make_case(name, c) for name, c in CASES.items()}
    assert cases['guard']['peak'] > 1.0
    assert cases['gap']['nsilent'] > 2 and cases['gap']['status'] == 0
    assert cases['zeros']['status'] == W.WHISPER_SILENT == cases['empty']['status']
    assert cases['empty_prev']['status'] == 0
    largest = {k: max(c['move'][k] for c in cases.values()) for k in ('r', 'a', 'sigma', 'y', 'peak')}
    for name, c in cases.items():
        print('{:11s} T={:5d} status={} nsilent={:2d} minorder={:2d} peak={:.4f} move y={:.2e} '
              'a={:.2e}'.format(name, len(c['x']), c['status'], c['nsilent'], c['minorder'],
                                c['peak'], c['move']['y'], c['move']['a']))
    print('largest movement', largest)
    torch.save(dict(cases=cases, largest_move=largest, max_move=MAX_MOVE), out)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'tests', 'golden', 'whisper.pt'))
