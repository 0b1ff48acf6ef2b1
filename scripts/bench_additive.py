"""Device time of the on-the-fly additive-noise mixer (ops.asl_p56 + ops.additive_mix, DESIGN.md
section 11) for one training batch, [300, 16384] speech-like rows at 16 kHz against a 60 s noise
bank, next to the host time per slice of the numpy oracle (scripts/additive_oracle.py; the
reference's own python loop is 0.07 - 0.15 s per slice and is not installed beside the GPU).

    python scripts/bench_additive.py [--bench-line FILE] > profiles/additive_bench.json

Each leg is warmed up, then timed with device events over `--reps` back-to-back calls (a window
of a few hundred ms) ending in a synchronise.  `--bench-line FILE`: the JSON line of a `bench.py
--precision bf16` run of the same session; the mixer has to cost less than that GAN step for the
loader's side stream to hide it, and the verdict is recorded.
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
    ap.add_argument('--reps', type=int, default=1000)
    ap.add_argument('--oracle-slices', type=int, default=20)
    ap.add_argument('--bench-line', default=None)
    args = ap.parse_args()
    import torch
    import additive_oracle as A
    from make_golden_additive import speech_like
    from segan_pytorch_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_additive.py measures on an MI355X: no HIP device is visible')
    rng = np.random.default_rng(0)
    base = speech_like(args.T * 8, 16000, 1)
    offs = rng.integers(0, len(base) - args.T, args.rows)
    scale = rng.uniform(0.2, 1.0, args.rows).astype(np.float32)
    X = np.stack([base[o:o + args.T] * s for o, s in zip(offs, scale)]).astype(np.float32)
    bank_h = (0.05 * rng.standard_normal(60 * 16000)).astype(np.float32)
    starts = rng.integers(1, len(bank_h) - args.T, args.rows)
    snrs = rng.choice([0.0, 5.0, 10.0], args.rows)
    x, bank = torch.from_numpy(X).cuda(), torch.from_numpy(bank_h).cuda()

    def both():
        lv = ops.asl_p56(x)
        return ops.additive_mix(x, bank, starts, snrs, lv['asl_ms'])

    def timed(fn, reps):
        for _ in range(10):
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

    lv = ops.asl_p56(x)
    px = lv['asl_ms'].contiguous()
    level_ms, _ = timed(lambda: ops.asl_p56(x), args.reps)
    mix_ms, _ = timed(lambda: ops.additive_mix(x, bank, starts, snrs, px), args.reps)
    both_ms, both_wall = timed(both, args.reps)
    noisy, info = both()
    t0 = time.perf_counter()
    for r in range(args.oracle_slices):
        o = A.asl_p56(X[r])
        A.mix(X[r], bank_h[starts[r]:starts[r] + args.T], snrs[r], o['asl_ms'])
    oracle_s = (time.perf_counter() - t0) / args.oracle_slices
    samples = args.rows * args.T
    out = {'what': 'ops.asl_p56 + ops.additive_mix, [{}, {}] fp32 rows, device events over {} calls '
                   'after warm-up'.format(args.rows, args.T, args.reps),
           'level_ms': level_ms, 'mix_ms_with_host_argument_copies': mix_ms,
           'level_plus_mix_ms': both_ms, 'level_plus_mix_host_wall_ms': both_wall,
           'msamples_per_s': samples / both_ms / 1e3,
           'bytes_moved_min': samples * 4 * 4,      # x read twice, segment read, noisy written
           'rows_mixed': int((info['sf'] > 0).sum()), 'divisions_max': int(info['n'].max()),
           'host_numpy_oracle_s_per_slice': oracle_s,
           'host_note': 'scripts/additive_oracle.py (vectorised fp64 numpy), one thread, measured in '
                        'this job; NOT the reference, whose per-sample python loop is not available '
                        'beside the GPU',
           'host_oracle_ms_per_batch_one_thread': 1e3 * oracle_s * args.rows}
    if args.bench_line:
        line = [l for l in open(args.bench_line).read().splitlines() if l.startswith('{')][-1]
        b = json.loads(line)
        out['gan_step_ms_same_session'] = b['ms_per_step']
        out['gan_step_precision'] = b.get('precision')
        out['below_one_gan_step'] = bool(both_ms < b['ms_per_step'])
        out['share_of_gan_step'] = both_ms / b['ms_per_step']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
