"""Writes tests/golden/rir.pt: the rooms of the GPU test of the room-impulse-response synthesis
 with what scripts/rir_oracle.py makes of them.

Per row: the geometry, the length, the response in float64, the image count, and `move`, the
largest |h64 - h80| between the oracle in float64 and in numpy.longdouble: the GPU test allows
100 times that.  `margin` is how far, in samples, the closest image is from changing the count; a
row whose margin is below MARGIN is refused, so the count on the device can be asserted equal.

The rows are the smallest that take every path of segan_rir.hip: lengths around one tile, a
response that ends before the direct path, several tiles, a small live room with many columns per
tile, a cube with the source at its centre (coincident images) and a dead wall, all walls dead,
source and receiver 0.1 m apart, 8 kHz, and a row cut by `lengths`.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import rir_oracle as R  # noqa: E402

MARGIN = 1e-9

ROOM = [5.0, 4.0, 3.0]
SRC = [1.2, 1.7, 1.1]
MIC = [3.4, 2.3, 1.6]
B81 = [0.81] * 6

# name -> (L, s, r, beta, T, srate, length)
ROWS = {
    'T255': (ROOM, SRC, MIC, B81, 255, 16000, 255),
    'T256': (ROOM, SRC, MIC, B81, 256, 16000, 256),
    'T257': (ROOM, SRC, MIC, B81, 257, 16000, 257),
    'T1': (ROOM, SRC, MIC, B81, 1, 16000, 1),
    'T2048': (ROOM, SRC, MIC, B81, 2048, 16000, 2048),
    'small_live': ([2.0, 1.6, 1.5], [0.5, 0.6, 0.7], [1.4, 1.0, 0.9], [0.95] * 6, 1024, 16000, 1024),
    'cube_centre': ([4.0, 4.0, 4.0], [2.0, 2.0, 2.0], [1.0, 2.5, 2.9],
                    [0.9, 0.7, 0.0, 0.85, 0.6, 0.95], 1500, 16000, 1500),
    'dead': (ROOM, SRC, MIC, [0.0] * 6, 300, 16000, 300),
    'near': (ROOM, SRC, [1.2, 1.76, 1.18], B81, 512, 16000, 512),
    'rate8': (ROOM, SRC, MIC, B81, 700, 8000, 700),
    'masked': (ROOM, SRC, MIC, B81, 600, 16000, 333),
}


def geom_of(row):
    L, s, r, beta = row[:4]
    return np.concatenate([np.asarray(v, np.float64) for v in (L, s, r, beta)])


def build():
    """The fixture; raises where a row's count could flip."""
    import torch
    rows = {}
    for name, row in ROWS.items():
        g = geom_of(row)
        T, srate, length = row[4:]
        a = R.rir_rows(g[None], T, srate, [length])
        b = R.rir_rows(g[None], T, srate, [length], dtype=np.longdouble)
        if a['margin'][0] < MARGIN:
            raise SystemExit('{}: an image is {} samples from changing the count'.format(
                name, a['margin'][0]))
        assert a['images'][0] == b['images'][0], name
        h = a['h'][0]
        rows[name] = {'geom': torch.from_numpy(g.copy()), 'T': T, 'srate': srate, 'length': length,
                      'h': torch.from_numpy(h.copy()), 'images': int(a['images'][0]),
                      'move': float(np.abs(b['h'][0] - h.astype(np.longdouble)).max()),
                      'peak': float(np.abs(h).max()), 'margin': float(a['margin'][0])}
    meta = {'recipe': 'scripts/make_golden_rir.py', 'oracle': 'scripts/rir_oracle.py',
            'margin_floor': MARGIN, 'numpy': np.__version__}
    return {'rows': rows, 'meta': meta}


def main(out):
    import torch
    fx = build()
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')
    for name, c in fx['rows'].items():
        print('  {:12s} T {:5d} images {:6d} peak {:.3e} move/peak {:.2e} margin {:.2e}'.format(
            name, c['T'], c['images'], c['peak'], c['move'] / c['peak'] if c['peak'] else 0.0,
            c['margin']))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'rir.pt'))
