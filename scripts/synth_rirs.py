#!/usr/bin/env python
"""Writes a fixed bank of synthetic room impulse responses: shoebox rooms
drawn by augment.draw_rooms from numpy.random.default_rng(seed), synthesised on the GPU by the
image-source method (ops.rir_shoebox).

    python scripts/synth_rirs.py --out DIR --count 64 --seed 0

DIR receives rir_0000.wav .. as float32 at --srate with the physical scale 1 / (4 pi d), row i
ceil(1.5 rt60_i srate) taps long (--max_taps at the most), and rooms.csv with one line per
response: file, taps, nominal rt60, beta, the room, the source and the receiver.  DIR is a valid
argument of train.py --reverb_rirs (the bank normalises each response by its direct path).
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS = ('file', 'taps', 'rt60', 'beta', 'Lx', 'Ly', 'Lz', 'sx', 'sy', 'sz', 'rx', 'ry', 'rz')


def build_parser():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--out', type=str, required=True, help='directory to write (created)')
    p.add_argument('--count', type=int, required=True, help='responses to write (1 .. 9999)')
    p.add_argument('--seed', type=int, required=True)
    p.add_argument('--srate', type=int, default=16000, choices=[16000, 8000])
    p.add_argument('--max_taps', type=int, default=16384)
    p.add_argument('--rt60', type=float, nargs=2, default=[0.2, 0.8], metavar=('LO', 'HI'))
    p.add_argument('--room_min', type=float, nargs=3, default=[3.0, 3.0, 2.5],
                   metavar=('X', 'Y', 'Z'))
    p.add_argument('--room_max', type=float, nargs=3, default=[10.0, 8.0, 4.0],
                   metavar=('X', 'Y', 'Z'))
    p.add_argument('--wall_margin', type=float, default=0.5)
    p.add_argument('--min_dist', type=float, default=0.5)
    return p


def rows_of(rooms, lengths):
    """the lines of rooms.csv, as lists of strings (repr: the numbers read back exactly)"""
    out = []
    for i, n in enumerate(lengths):
        nums = [rooms['rt60'][i], rooms['beta'][i, 0]] + list(rooms['room'][i]) + list(
            rooms['src'][i]) + list(rooms['mic'][i])
        out.append(['rir_{:04d}.wav'.format(i), str(int(n))] + [repr(float(v)) for v in nums])
    return out


def main(opts):
    if not 1 <= opts.count <= 9999:
        raise SystemExit('--count must lie in 1 .. 9999, got {}'.format(opts.count))
    if opts.max_taps < 1:
        raise SystemExit('--max_taps must be positive, got {}'.format(opts.max_taps))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('segan_pytorch_amd runs only on an MI355X (HIP) device: no GPU is visible '
                         '(and there is no CPU fallback)')
    from scipy.io import wavfile
    from segan_pytorch_amd import augment, ops
    try:
        rooms = augment.draw_rooms(np.random.default_rng(opts.seed), opts.count, rt60=opts.rt60,
                                   room_min=opts.room_min, room_max=opts.room_max,
                                   wall_margin=opts.wall_margin, min_dist=opts.min_dist)
    except ValueError as e:
        raise SystemExit(str(e))
    lengths = np.minimum(opts.max_taps, np.ceil(1.5 * rooms['rt60'] * opts.srate)).astype(np.int64)
    h = ops.rir_shoebox(rooms['room'], rooms['src'], rooms['mic'], rooms['beta'],
                        int(lengths.max()), srate=opts.srate, lengths=lengths).cpu().numpy()
    os.makedirs(opts.out, exist_ok=True)
    for i, n in enumerate(lengths):
        wavfile.write(os.path.join(opts.out, 'rir_{:04d}.wav'.format(i)), opts.srate,
                      h[i, :n].astype(np.float32))
    with open(os.path.join(opts.out, 'rooms.csv'), 'w', newline='') as f:
        w = csv.writer(f)
        w.writerow(COLUMNS)
        w.writerows(rows_of(rooms, lengths))
    print('wrote {} responses of {} .. {} taps and rooms.csv to {}'.format(
        opts.count, int(lengths.min()), int(lengths.max()), opts.out))


if __name__ == '__main__':
    main(build_parser().parse_args())
