"""Throughput of the room-impulse-response synthesis (ops.rir_shoebox) on the
--rooms rooms that augment.draw_rooms gives at seed 0, --taps samples each at 16 kHz; prints one
JSON line and writes it to --out (profiles/rir_bench.json).

    python scripts/bench_rir.py            # MI355X

One warm-up call, then --reps timed calls between device events (mean, smallest, largest), the
images of all rooms per second, whether two calls give the same bits, and the wall time of
RIRBank.synthetic for the same rooms (rows of 1.5 rt60, normalisation on the host included).  The
numpy oracle scripts/rir_oracle.py is timed on the host on the --cpu rooms with the fewest images,
with its largest distance from the device's result on those.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', type=int, default=1)
    ap.add_argument('--rooms', type=int, default=64)
    ap.add_argument('--taps', type=int, default=16384)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rir_bench.json'))
    args = ap.parse_args()
    import torch
    import rir_oracle
    from bench_denoise import timed
    from segan_pytorch_amd import augment, ops
    rooms = augment.draw_rooms(np.random.default_rng(0), args.rooms)
    geo = (rooms['room'], rooms['src'], rooms['mic'], rooms['beta'])
    st = ops.rir_stages(*geo, args.taps)
    images = st['images'].cpu().numpy()
    h, ms = timed(torch, lambda: ops.rir_shoebox(*geo, args.taps), args.reps)
    mean = float(np.mean(ms))
    out = {'leg': 'mi355x', 'op': 'rir_shoebox', 'rooms': args.rooms, 'taps': args.taps,
           'srate': 16000, 'seed': 0, 'reps': args.reps, 'images_total': int(images.sum()),
           'images_min': int(images.min()), 'images_max': int(images.max()),
           'mean_ms': mean, 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)),
           'ms_per_response': mean / args.rooms, 'images_per_s': float(images.sum()) / (mean / 1e3),
           'same_bits': bool(torch.equal(h.view(torch.int64), st['h'].view(torch.int64)))}
    t0 = time.perf_counter()
    bank = augment.RIRBank.synthetic(args.rooms, seed=0, device='cuda', max_taps=args.taps)
    out['bank_synthesis_s'] = time.perf_counter() - t0
    out['bank_taps_mean'] = float(bank.taps.mean())
    few = np.argsort(images, kind='stable')[:args.cpu]
    secs, diff = [], 0.0
    for i in few:
        t0 = time.perf_counter()
        o = rir_oracle.rir(rooms['room'][i], rooms['src'][i], rooms['mic'][i], rooms['beta'][i],
                           args.taps)
        secs.append(time.perf_counter() - t0)
        assert o['images'] == images[i], (o['images'], images[i])
        diff = max(diff, float(np.abs(h[i].cpu().numpy() - o['h']).max() / np.abs(o['h']).max()))
    out['oracle_cpu_rooms'] = [int(i) for i in few]
    out['oracle_cpu_images'] = [int(images[i]) for i in few]
    out['oracle_cpu_s_per_response'] = float(np.mean(secs)) if secs else None
    out['max_diff_vs_oracle_rel_peak'] = diff
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
