"""Device time of the on-the-fly distortions (ops.clip_rows, ops.chop_rows, ops.fir_rows,
augment.Distort) for one training batch, [300, 16384] fp32 rows, next to the
numpy oracle's host time per row on one thread (scripts/distort_oracle.py), all in one job.

    python scripts/bench_distort.py > profiles/distort_bench.json

Each leg is warmed up, then timed with device events over `--reps` back-to-back calls ending in a
synchronise.  Legs: the clip; the P.56 level with its envelope (what the chop needs first) and the
chop kernel alone; the FIR with every row on one filter, per default cutoff (K = 256, 128, 64) and
at the longest filter the kernel takes (K = 2048); `Clip.apply`, `Chop.apply`, `BandLimit.apply`
and the default mix `Distort.apply` as the loader calls them (draws, allocations, pinned uploads,
the gathers and scatters of the mix included; host wall time per call beside the device time).
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
    ap.add_argument('--rows', type=int, default=300)
    ap.add_argument('--T', type=int, default=16384)
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--oracle-rows', type=int, default=3)
    args = ap.parse_args()
    import torch
    import distort_oracle as D
    import make_golden_additive as GA
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_distort.py measures on an MI355X: no HIP device is visible')
    rows, T = args.rows, args.T
    rng = np.random.default_rng(0)
    base = np.stack([GA.speech_like(T, 16000, 200 + i) for i in range(8)])
    X = base[rng.integers(8, size=rows)] * rng.uniform(0.5, 1.5, (rows, 1)).astype(np.float32)
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    prev = torch.from_numpy((0.1 * rng.standard_normal(rows)).astype(np.float32)).cuda()

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, 1e3 * (time.perf_counter() - t0) / reps

    clip, chop, band = A.Clip(seed=1), A.Chop(seed=1), A.BandLimit(seed=1)
    out = {'what': 'clip / chop / band limiting of [{}, {}] fp32 rows, device events over {} calls '
                   'after warm-up'.format(rows, T, args.reps), 'device_ms': {}, 'apply_ms': {}}
    dev = out['device_ms']
    f_d = torch.from_numpy(clip.draw(rng, rows)).cuda()
    dev['clip_rows'] = timed(lambda: ops.clip_rows(x, f_d, None, prev), args.reps)[0]
    dev['asl_p56_stages'] = timed(lambda: ops.asl_p56_stages(x), args.reps)[0]
    level = ops.asl_p56_stages(x)
    u, dur = chop.draw(rng, rows)
    u_d, dur_d = torch.from_numpy(u).cuda(), torch.from_numpy(dur).cuda()
    dev['chop_rows'] = timed(lambda: ops.chop_rows(x, level['q'], level['c0'], u_d, dur_d),
                             args.reps)[0]
    bank, K = band.data('cuda')
    for f, fc in enumerate(band.cutoffs):
        ids = torch.full((rows,), f, dtype=torch.int32, device='cuda')
        dev['fir_rows_K{}'.format(int(band.K[f]))] = timed(
            lambda: ops.fir_rows(x, bank, K, ids, None, prev), args.reps)[0]
    long_b, long_K = A.BandLimit((125.0,)).data('cuda')
    ids0 = torch.zeros(rows, dtype=torch.int32, device='cuda')
    dev['fir_rows_K2048'] = timed(lambda: ops.fir_rows(x, long_b, long_K, ids0, None, prev),
                                  max(10, args.reps // 10))[0]
    flops = rows * (T + 1) * 3.0
    out['fir_gflops'] = {k: flops * int(k.split('K')[1]) / v / 1e6 for k, v in dev.items()
                         if k.startswith('fir_rows_K')}
    mix = A.Distort([clip, chop, band], seed=1)
    for name, obj in (('Clip', clip), ('Chop', chop), ('BandLimit', band), ('Distort', mix)):
        d, h = timed(lambda: obj.apply(x, prev=prev), args.reps)
        out['apply_ms'][name] = {'device': d, 'host_wall': h}

    # the numpy oracle, one thread, per row
    n = args.oracle_rows
    Ks, h = D.lowpass(1000.0)
    t0 = time.perf_counter()
    for r in range(n):
        D.clip(X[r], 0.3, None, 0.1)
    t1 = time.perf_counter()
    import additive_oracle as AO
    for r in range(n):
        o = AO.asl_p56(X[r])
        D.chop(X[r], o['q'], o['c0'], u[r], dur[r])
    t2 = time.perf_counter()
    for r in range(n):
        D.fir(X[r], h, None, 0.1)
    t3 = time.perf_counter()
    out['host_numpy_oracle_ms_per_row'] = {'clip': 1e3 * (t1 - t0) / n,
                                           'chop_with_level': 1e3 * (t2 - t1) / n,
                                           'fir_K256': 1e3 * (t3 - t2) / n}
    # parity of the timed outputs, a few rows
    y, info = ops.fir_rows(x, bank, K, torch.zeros(rows, dtype=torch.int32, device='cuda'), None,
                           prev, torch.float64)
    yo, po = D.fir(X[0], h, None, float(prev[0]))
    out['fir_fp64_bit_equal_row0'] = bool(np.array_equal(y[0].cpu().numpy(), yo) and
                                          float(info['prev'][0]) == po)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
