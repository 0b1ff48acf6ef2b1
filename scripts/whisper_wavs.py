"""Writes a fixed whispered copy of a directory of wavs: every IN_DIR/*.wav
resynthesised on the GPU as pseudo-whisper (noise-excited LPC: `augment.Whisper`), under the same
file name in OUT_DIR — a test set on disk for the evaluation CLI, which reads directories.

    python scripts/whisper_wavs.py IN_DIR OUT_DIR --seed 0 [--tilts 0.0 0.5 0.9] [--lag_hz 120]

The draws (a noise seed and a tilt per file) come from one generator seeded with `--seed` and the
files are taken in sorted order, so the same command writes the same files.  16-bit PCM in and out
(int16 / 32768, rounded half to even and saturated on the way back); multi-channel files are
averaged.  Files are processed one by one: each is its own row, whatever its length.  The rate must
be 16000: the frame, the order and the lag window are defined at that rate.  OUT_DIR/whisper.json
records what was done to each file.
"""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRATE = 16000


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('in_dir')
    ap.add_argument('out_dir')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--tilts', type=float, nargs='+', default=[0.0, 0.5, 0.9])
    ap.add_argument('--lag_hz', type=float, default=120.0)
    args = ap.parse_args(argv)
    names = sorted(glob.glob(os.path.join(args.in_dir, '*.wav')))
    if not names:
        raise SystemExit('no wavs found in {}'.format(args.in_dir))
    import torch
    from scipy.io import wavfile
    from segan_pytorch_amd import augment
    if not torch.cuda.is_available():
        raise SystemExit('whisper_wavs.py runs on an MI355X: no HIP device is visible')
    whisper = augment.Whisper(args.tilts, args.lag_hz)
    rng = np.random.default_rng(args.seed)
    os.makedirs(args.out_dir, exist_ok=True)
    log = {}
    for path in names:
        rate, w = wavfile.read(path)
        if rate != SRATE:
            raise SystemExit('{} is at {} Hz, not {}'.format(path, rate, SRATE))
        if w.dtype != np.int16:
            raise SystemExit('{} is {}, not 16-bit PCM'.format(path, w.dtype))
        x = w.astype(np.float32) / np.float32(32768)
        if x.ndim == 2:
            x = x.mean(axis=1)
        out, info = whisper.apply(torch.from_numpy(np.ascontiguousarray(x[None])).cuda(),
                                  generator=rng)
        y = np.rint(out[0].double().cpu().numpy() * 32768.0)
        base = os.path.basename(path)
        wavfile.write(os.path.join(args.out_dir, base), rate,
                      np.clip(y, -32768, 32767).astype(np.int16))
        log[base] = {'seed': int(info['seeds'][0]), 'tilt': float(info['tilts'][0]),
                     'status': int(info['status'][0]), 'nsilent': int(info['nsilent'][0]),
                     'minorder': int(info['minorder'][0]), 'peak': float(info['peak'][0])}
    with open(os.path.join(args.out_dir, 'whisper.json'), 'w') as f:
        json.dump({'seed': args.seed, 'tilts': args.tilts, 'lag_hz': args.lag_hz, 'files': log}, f,
                  indent=1)
    print('wrote {} files to {}'.format(len(names), args.out_dir))


if __name__ == '__main__':
    main()
