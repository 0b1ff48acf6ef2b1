"""Device time of ops.resample for a batch of 256 rows of 4 s, int16 ->
int16, 48 kHz -> 16 kHz and 44.1 kHz -> 16 kHz at the default filter (32, 8.6), next to
scipy.signal.resample_poly on one host thread over a subset of the same rows.

    python scripts/bench_resample.py > profiles/resample_bench.json

Each leg is warmed up (the first call also builds and uploads the tap table), then timed with
device events over `--reps` back-to-back calls ending in a synchronise.  Reported per leg: ms per
call, bytes read + written per second against the 6.29 TB/s device-copy figure, and the fp64 FMA
rate (one FMA per product of the polyphase sum).  Nothing is gated on these figures: the
conversion is a capability, scipy converts a 3 s utterance in a few ms on one core.
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

COPY_TBPS = 6.29


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=256)
    ap.add_argument('--seconds', type=float, default=4.0)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--host-rows', type=int, default=8)
    args = ap.parse_args()
    import torch
    from scipy.signal import resample_poly
    import resample_oracle as R
    from segan_pytorch_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample.py measures on an MI355X: no HIP device is visible')
    os.environ.setdefault('OMP_NUM_THREADS', '1')
    rng = np.random.default_rng(0)
    legs = []
    for rate_in, rate_out in ((48000, 16000), (44100, 16000)):
        T = int(round(args.seconds * rate_in))
        X = rng.integers(-12000, 12001, size=(args.rows, T)).astype(np.int16)
        x = torch.from_numpy(X).cuda()
        p, q, taps = R.plan(rate_in, rate_out)
        for _ in range(3):
            y, info = ops.resample(x, rate_in, rate_out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.reps):
            y, info = ops.resample(x, rate_in, rate_out)
        e1.record()
        torch.cuda.synchronize()
        ms, wall_ms = e0.elapsed_time(e1) / args.reps, 1e3 * (time.perf_counter() - t0) / args.reps
        Ly = y.shape[1]
        # products of the polyphase sum: every output meets the taps of its phase (row edges ignored)
        fma = args.rows * Ly * (len(taps) / p)
        nbytes = 2 * args.rows * (T + Ly)
        t0 = time.perf_counter()
        host = [resample_poly(X[r].astype(np.float64), p, q, window=taps / p)
                for r in range(args.host_rows)]
        host_s = (time.perf_counter() - t0) / args.host_rows
        got = y[:args.host_rows].cpu().numpy()
        want = np.stack([R.to_int16(h)[0] for h in host])
        legs.append({'rate_in': rate_in, 'rate_out': rate_out, 'p': p, 'q': q, 'taps': len(taps),
                     'rows': args.rows, 'T': T, 'Ly': Ly, 'ms_per_call': ms,
                     'host_wall_ms_per_call': wall_ms,
                     'gbytes_per_s_in_plus_out': nbytes / ms / 1e6,
                     'share_of_copy_rate': nbytes / ms / 1e9 / COPY_TBPS,
                     'fp64_gfma_per_s': fma / ms / 1e6,
                     'utterances_per_s': args.rows / ms * 1e3,
                     'saturated_samples': int(info['nclip'].sum()),
                     'scipy_resample_poly_ms_per_row_one_thread': 1e3 * host_s,
                     'scipy_ms_for_the_batch_one_thread': 1e3 * host_s * args.rows,
                     'int16_samples_differing_from_scipy': int((got != want).sum())})
    print(json.dumps({'what': 'ops.resample int16 -> int16, zeros=32 beta=8.6, device events over {} '
                              'calls after warm-up'.format(args.reps),
                      'copy_rate_tbps_reference': COPY_TBPS, 'legs': legs}))


if __name__ == '__main__':
    main()
