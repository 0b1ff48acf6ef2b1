"""Writes a fixed distorted copy of a directory of wavs: every IN_DIR/*.wav
clipped, with chunks of speech removed or band limited on the GPU, under the same file name in
OUT_DIR — a test set on disk for the evaluation CLI, which reads directories.

    python scripts/distort_wavs.py IN_DIR OUT_DIR --kind clip [chop bandlimit] --seed 0

With several kinds each file gets one of them, drawn uniformly (`augment.Distort`).  The draws come
from one generator seeded with `--seed` and the files are taken in sorted order, so the same
command writes the same files.  16-bit PCM in and out (int16 / 32768, rounded half to even and
saturated on the way back); multi-channel files are averaged.  Files are processed one by one: each
is its own row, whatever its length.  The rate must be `--srate` (16000): the chop's level and the
cutoffs are defined at that rate.  OUT_DIR/distort.json records what was done to each file.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('in_dir')
    ap.add_argument('out_dir')
    ap.add_argument('--kind', nargs='+', required=True, choices=['clip', 'chop', 'bandlimit'])
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--srate', type=int, default=16000)
    ap.add_argument('--clip_factors', type=float, nargs='+', default=[0.1, 0.2, 0.3, 0.4, 0.5])
    ap.add_argument('--chop_max', type=int, default=3)
    ap.add_argument('--chop_durs', type=float, nargs=2, default=[0.05, 0.3])
    ap.add_argument('--bandlimit_cutoffs', type=float, nargs='+', default=[1000, 2000, 4000])
    args = ap.parse_args(argv)
    if len(set(args.kind)) != len(args.kind):
        raise SystemExit('--kind names a kind twice')
    names = sorted(glob.glob(os.path.join(args.in_dir, '*.wav')))
    if not names:
        raise SystemExit('no wavs found in {}'.format(args.in_dir))
    import torch
    from scipy.io import wavfile
    from segan_pytorch_amd import augment
    if not torch.cuda.is_available():
        raise SystemExit('distort_wavs.py runs on an MI355X: no HIP device is visible')
    make = {'clip': lambda: augment.Clip(args.clip_factors),
            'chop': lambda: augment.Chop(args.chop_max, args.chop_durs, args.srate),
            'bandlimit': lambda: augment.BandLimit(args.bandlimit_cutoffs, args.srate)}
    distort = augment.Distort({k: make[k]() for k in args.kind})
    rng = np.random.default_rng(args.seed)
    os.makedirs(args.out_dir, exist_ok=True)
    log = {}
    for path in names:
        rate, w = wavfile.read(path)
        if rate != args.srate:
            raise SystemExit('{} is at {} Hz, not {}'.format(path, rate, args.srate))
        if w.dtype != np.int16:
            raise SystemExit('{} is {}, not 16-bit PCM'.format(path, w.dtype))
        x = w.astype(np.float32) / np.float32(32768)
        if x.ndim == 2:
            x = x.mean(axis=1)
        out, info = distort.apply(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(),
                                  generator=rng)
        y = np.rint(out[0].double().cpu().numpy() * 32768.0)
        base = os.path.basename(path)
        wavfile.write(os.path.join(args.out_dir, base), rate,
                      np.clip(y, -32768, 32767).astype(np.int16))
        kind = str(info['kinds'][0])
        sub = info[kind]
        rec = {'kind': kind, 'status': int(info['status'][0])}
        if kind == 'clip':
            rec.update(factor=float(sub['factors'][0]), nclipped=int(sub['nclipped'][0]))
        elif kind == 'chop':
            rec.update(starts=sub['starts'][0].tolist(), dur=sub['dur'][0].tolist(),
                       nzeroed=int(sub['nzeroed'][0]))
        else:
            rec.update(cutoff=float(sub['cutoffs'][0]))
        log[base] = rec
    with open(os.path.join(args.out_dir, 'distort.json'), 'w') as f:
        json.dump({'seed': args.seed, 'kinds': args.kind, 'files': log}, f, indent=1)
    print('wrote {} files to {}'.format(len(names), args.out_dir))


if __name__ == '__main__':
    main()
