"""Device time of the on-the-fly whisper (ops.whisper_rows, augment.Whisper)
for one training batch, [300, 16384] fp32 rows, next to the numpy oracle's host time per row on one
thread (scripts/whisper_oracle.py), all in one job.

    python scripts/bench_whisper.py > profiles/whisper_bench.json

Each leg is warmed up, then timed with device events over `--reps` back-to-back calls ending in a
synchronise.  Legs: the lags; the Levinson recursion; the synthesis with its overlap-add (the two
kernels of `segan_whisper_synth`); the whole `ops.whisper_rows` with device-resident arguments;
`Whisper.apply` as the loader calls it (draws, allocations and pinned uploads included; host wall
time per call beside the device time).  The rows are the periodic test signal of the oracle.  No
time is asserted anywhere: there is no earlier figure to hold these against.
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
    import whisper_oracle as W
    from segan_pytorch_amd import _lib
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_whisper.py measures on an MI355X: no HIP device is visible')
    rows, T = args.rows, args.T
    rng = np.random.default_rng(0)
    base = np.stack([W.voiced(f0, T, f0) for f0 in (95, 110, 140, 180, 210, 240, 270, 300)])
    X = base[rng.integers(8, size=rows)] * rng.uniform(0.5, 1.5, (rows, 1)).astype(np.float32)
    x = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda()
    prev = torch.from_numpy((0.01 * rng.standard_normal(rows)).astype(np.float32)).cuda()

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

    wh = A.Whisper(seed=1)
    seeds, ids = wh.draw(rng, rows)
    s_d = torch.from_numpy(seeds).cuda()
    t_d = torch.from_numpy(wh.tilts[ids]).cuda()
    out = {'what': 'noise-excited LPC resynthesis of [{}, {}] fp32 rows, device events over {} '
                   'calls after warm-up'.format(rows, T, args.reps), 'device_ms': {}, 'apply_ms': {}}
    dev = out['device_ms']
    lib = _lib.load()
    st = ops.whisper_stages(x, s_d, t_d, None, prev)
    w, g = ops._whisper_tables(x.device, 120.0)
    F = ops.whisper_frames(T)
    ws = torch.empty(rows * ops.WHISPER_N * F, device='cuda', dtype=torch.float64)
    y = torch.empty_like(x)
    po = torch.empty(rows, device='cuda')
    pk = torch.empty(rows, device='cuda', dtype=torch.float64)
    i1, i2, i3 = (torch.empty(rows, device='cuda', dtype=torch.int32) for _ in range(3))
    P, S = ops._ptr, ops._stream
    dev['whisper_lags'] = timed(lambda: _lib.check(lib.segan_whisper_lags(
        P(x), None, P(prev), P(w), P(g), rows, T, P(st['r']), S())), args.reps)[0]
    dev['whisper_lpc'] = timed(lambda: ops.whisper_lpc(st['r']), args.reps)[0]
    dev['whisper_synth_and_ola'] = timed(lambda: _lib.check(lib.segan_whisper_synth(
        P(x), None, P(prev), P(st['r']), P(st['a']), P(st['sigma']), P(st['order']), P(s_d), P(t_d),
        P(w), rows, T, P(ws), ws.numel(), P(y), 0, P(po), P(pk), P(i1), P(i2), P(i3), S())),
        args.reps)[0]
    dev['whisper_rows'] = timed(lambda: ops.whisper_rows(x, s_d, t_d, None, prev), args.reps)[0]
    d, h = timed(lambda: wh.apply(x, prev=prev), args.reps)
    out['apply_ms']['Whisper'] = {'device': d, 'host_wall': h}
    out['workspace_bytes'] = int(lib.segan_whisper_ws_doubles(rows, T)) * 8

    n = args.oracle_rows
    t0 = time.perf_counter()
    for r in range(n):
        o = W.whisper(X[r], int(seeds[r]), float(wh.tilts[ids[r]]), None, float(prev[r]))
    out['host_numpy_oracle_ms_per_row'] = 1e3 * (time.perf_counter() - t0) / n
    # parity of the timed output, the last oracle row
    y64, info = ops.whisper_rows(x, s_d, t_d, None, prev, torch.float64)
    r = n - 1
    out['fp64_bit_equal_oracle_row'] = bool(np.array_equal(y64[r].cpu().numpy(), o['out']) and
                                            float(info['prev'][r]) == float(o['prev_out']))
    out['rows_with_peak_guard'] = int((info['peak'] > 1).sum())
    out['min_order'] = int(info['minorder'].min())
    print(json.dumps(out))


if __name__ == '__main__':
    main()
