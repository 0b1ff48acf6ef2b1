"""Device time of the on-the-fly reverberation (ops.reverb_rows) for one
training batch, [300, 16384] fp32 rows against room impulse responses of 4000 and of 16384 taps,
stage by stage (staging, forward transform, delay line, inverse transform, output stage), next to
the numpy oracle's host time per slice on one thread (scripts/reverb_oracle.py) and to a plain
torch.fft route over the same rows (rfft of the zero-padded rows, one product with the responses'
precomputed full-length spectra gathered per row, irfft, shift), all in one job.

    python scripts/bench_reverb.py > profiles/reverb_bench.json

Each leg is warmed up, then timed with device events over `--reps` back-to-back calls ending in a
synchronise.  The stage legs call the library's separate entry points on preallocated buffers; the
`rows` leg is `ops.reverb_rows` as the loader calls it (allocations and the pinned upload of the
ids included).
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
    ap.add_argument('--taps', type=int, nargs='+', default=[4000, 16384])
    ap.add_argument('--rirs', type=int, default=8)
    ap.add_argument('--reps', type=int, default=1000)
    ap.add_argument('--oracle-slices', type=int, default=3)
    ap.add_argument('--partition', type=int, default=None,
                    help='the partition of a library built with -DSEGAN_REVERB_P=N (loaded through '
                         '$SEGAN_HIP_LIB): the python side follows it')
    args = ap.parse_args()
    import torch
    import reverb_oracle as R
    from segan_pytorch_amd import _lib, ops
    from segan_pytorch_amd.augment import RIRBank
    from segan_pytorch_amd.ops import _ptr, _stream
    if not torch.cuda.is_available():
        raise SystemExit('bench_reverb.py measures on an MI355X: no HIP device is visible')
    lib = _lib.load()
    if args.partition is not None:
        ops.REVERB_P = args.partition
    assert ops.reverb_dims(1, 1, 0)['P'] == ops.REVERB_P, 'the library was built for another partition'
    rng = np.random.default_rng(0)
    rows, T, P = args.rows, args.T, ops.REVERB_P
    X = (0.3 * rng.standard_normal((rows, T))).astype(np.float32)
    x = torch.from_numpy(X).cuda()
    prev = torch.from_numpy((0.3 * rng.standard_normal(rows)).astype(np.float32)).cuda()

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

    out = {'what': 'ops.reverb_rows, [{}, {}] fp32 rows, partition {}, device events over {} calls '
                   'after warm-up; {} responses per bank, drawn uniformly per row'.format(
                       rows, T, P, args.reps, args.rirs), 'taps': {}}
    for taps in args.taps:
        hs = []
        for i in range(args.rirs):
            h = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.0)) * 0.2
            h[20 + i] = 1.0
            hs.append(h)
        bank = RIRBank(hs, max_taps=taps)
        ids_h = rng.integers(len(bank), size=rows)
        data = bank.data('cuda')
        ids = torch.from_numpy(ids_h.astype(np.int32)).cuda()
        fwd, inv = ops.reverb_basis('cuda')
        d = ops.reverb_dims(rows, T, data.max_delay)
        NB, M = d['blocks'], d['frames']
        xs = torch.empty(d['staging'], device='cuda')
        Xf = torch.empty((M, 2 * P), device='cuda')
        Yf = torch.empty((M, 2 * P), device='cuda')
        yt = torch.empty((M, P), device='cuda')
        y = torch.empty_like(x)
        pout = torch.empty(rows, device='cuda')
        status = torch.empty(rows, device='cuda', dtype=torch.int32)
        nparts, ntab = data.H.shape[0], data.table.shape[0]
        legs = {
            'stage': lambda: lib.segan_reverb_stage(_ptr(x), None, _ptr(prev), _ptr(xs), rows, T, NB,
                                                    M, _stream()),
            'forward_gemm': lambda: lib.segan_reverb_forward(_ptr(xs), _ptr(fwd), _ptr(Xf), M,
                                                             _stream()),
            'delay_line': lambda: lib.segan_reverb_fdl(_ptr(Xf), _ptr(data.H), nparts, _ptr(ids),
                                                       _ptr(data.table), ntab, _ptr(Yf), rows, T,
                                                       NB, M, _stream()),
            'inverse_gemm': lambda: lib.segan_reverb_inverse(_ptr(Yf), _ptr(inv), _ptr(yt), M,
                                                             _stream()),
            'output': lambda: lib.segan_reverb_finish(_ptr(yt), _ptr(x), None, _ptr(prev), nparts,
                                                      _ptr(ids), _ptr(data.table), ntab, _ptr(y),
                                                      _ptr(pout), _ptr(status), rows, T, NB, M,
                                                      _stream()),
        }
        res = {'blocks_per_row': NB, 'frames': M, 'partitions_per_rir': int(bank.partitions[0]),
               'bank_bytes_per_rir': int(bank.partitions[0]) * 2 * P * 4,
               'workspace_mbytes': d['workspace'] * 4 / 1e6, 'stages_ms': {}}
        for name, fn in legs.items():      # in chain order: every leg leaves its successor's input
            assert fn() == 0, name
            res['stages_ms'][name] = timed(fn, args.reps)[0]
        res['stages_sum_ms'] = sum(res['stages_ms'].values())
        res['rows_ms'], res['rows_host_wall_ms'] = timed(
            lambda: ops.reverb_rows(x, data, ids_h, None, prev), args.reps)
        # complex products of the delay line: sum over output blocks a of min(a + 1, partitions)
        npr = int(bank.partitions[0])
        pairs = sum(min(a + 1, npr) for a in range(NB))
        res['delay_line_gflops'] = rows * pairs * P * 8 / res['stages_ms']['delay_line'] / 1e6

        # the plain torch.fft route: full-length spectra of the responses precomputed
        nfft = 1 << int(np.ceil(np.log2(T + 1 + taps)))
        Hfull = torch.fft.rfft(torch.from_numpy(np.stack(bank.rirs)).cuda(), n=nfft)
        ids64 = ids.long()
        dl = torch.from_numpy(bank.delays[ids_h]).cuda()
        col = torch.arange(T + 1, device='cuda')[None, :] + dl[:, None]

        def fft_route():
            xe = torch.cat((prev[:, None], x), 1)
            Y = torch.fft.rfft(xe, n=nfft) * Hfull.index_select(0, ids64)
            full = torch.fft.irfft(Y, n=nfft)
            return full.gather(1, col)

        res['torch_fft_ms'] = timed(fft_route, max(50, args.reps // 10))[0]
        res['no_slower_than_torch_fft'] = bool(res['rows_ms'] <= res['torch_fft_ms'])
        yy, info = ops.reverb_rows(x, data, ids_h, None, prev)
        ref = fft_route()
        worst = 0.0
        for r in range(args.oracle_slices):
            h, dd = bank.rirs[ids_h[r]], int(bank.delays[ids_h[r]])
            yo, po = R.reverb(X[r], h, dd, None, float(prev[r]))
            s = R.scale(X[r], h, dd, None, float(prev[r]))
            worst = max(worst, float(np.abs(yy[r].cpu().numpy() - yo).max()) / s)
            res.setdefault('torch_fft_E', 0.0)
            res['torch_fft_E'] = max(res['torch_fft_E'],
                                     float(np.abs(ref[r, 1:].cpu().numpy() - yo).max()) / s)
        t0 = time.perf_counter()
        for r in range(args.oracle_slices):
            R.reverb(X[r], bank.rirs[ids_h[r]], int(bank.delays[ids_h[r]]), None, float(prev[r]))
        oracle_s = (time.perf_counter() - t0) / args.oracle_slices
        res['E_against_oracle'] = worst
        res['host_numpy_oracle_s_per_slice'] = oracle_s
        res['host_oracle_ms_per_batch_one_thread'] = 1e3 * oracle_s * rows
        out['taps'][str(taps)] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
