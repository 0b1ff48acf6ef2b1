"""Throughput of the WPE dereverberation baseline (ops.wpe_rows) over the 824 seeded synthetic
utterances of 1.5 - 4 s at 16 kHz that the other quality benches use (bench_quality.py), padded to
the longest with `lengths`; prints one JSON line and writes it to --out (profiles/wpe_bench.json).

    python scripts/bench_wpe.py            # MI355X

With the default parameters (10 taps, delay 3, 3 iterations): one call chunked under the default
workspace cap, and one call with a cap that takes the whole set at once; one warm-up call each,
then --reps timed calls between device events (mean, smallest, largest), and whether the two give
the same bits.  `taps32` is the chunked call with 32 taps.  The numpy oracle scripts/wpe_oracle.py
is timed per utterance on the first --cpu utterances on the host, with its largest distance from
the device's result on those.  `fixture` holds the SRMR (quality.srmr) of the fixture's two
reverberant signals before and after.  No time is asserted anywhere.
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

from bench_denoise import spread, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', type=int, default=3)
    ap.add_argument('--utts', type=int, default=824)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wpe_bench.json'))
    args = ap.parse_args()
    import torch
    import make_golden_wpe as GW
    import wpe_oracle
    from bench_quality import utterances
    from segan_pytorch_amd import ops, quality
    utts = utterances(args.utts)
    lengths = [len(d) for _, d in utts]
    deg = torch.zeros(len(utts), max(lengths))
    for i, (_, d) in enumerate(utts):
        deg[i, :len(d)] = torch.from_numpy(d)
    deg = deg.cuda()
    per_row = ops.wpe_dims(1, max(lengths))['ws_bytes']
    whole = per_row * len(utts) + 64
    out = {'leg': 'mi355x', 'op': 'wpe_rows', 'utts': len(utts),
           'mean_audio_s': float(np.mean(lengths)) / 16000, 'reps': args.reps,
           'taps': 10, 'delay': 3, 'iterations': 3,
           'ws_cap_bytes': ops.WPE_WS_CAP, 'ws_bytes_per_row': per_row,
           'calls_under_cap': -(-len(utts) // max(1, ops.WPE_WS_CAP // per_row)),
           'one_call_ws_bytes': whole, 'oracle_cpu_utts': args.cpu}
    y, ms = timed(torch, lambda: ops.wpe_rows(deg, lengths=lengths, out_dtype=torch.float64),
                  args.reps)
    y1, ms1 = timed(torch, lambda: ops.wpe_rows(deg, lengths=lengths, out_dtype=torch.float64,
                                                ws_cap=whole), args.reps)
    out['chunked'] = spread(ms, len(utts))
    out['one_call'] = spread(ms1, len(utts))
    out['same_bits'] = bool(torch.equal(y.view(torch.int64), y1.view(torch.int64)))
    del y1
    _, ms32 = timed(torch, lambda: ops.wpe_rows(deg, lengths=lengths, taps=32,
                                                out_dtype=torch.float64), args.reps)
    out['taps32'] = {'chunked': spread(ms32, len(utts))}
    t0 = time.perf_counter()
    want = [wpe_oracle.wpe(d, 16000)['y'] for _, d in utts[:args.cpu]]
    out['oracle_cpu_s_per_utt'] = (time.perf_counter() - t0) / max(args.cpu, 1)
    out['max_diff_vs_oracle_rel_peak'] = max(
        [float(np.abs(y[i, :len(w)].cpu().numpy() - w).max() / np.abs(utts[i][1]).max())
         for i, w in enumerate(want)] or [0.0])
    fx = torch.load(os.path.join(ROOT, 'tests', 'golden', 'wpe.pt'), map_location='cpu',
                    weights_only=False)
    scores = {}
    for name in ('rev03', 'rev06'):
        x = torch.from_numpy(GW.row(fx['signals'][name].numpy())).cuda()
        scores[name] = {'srmr_before': float(quality.srmr(x)[0]),
                        'srmr_after': float(quality.srmr(ops.wpe_rows(x))[0])}
    out['fixture'] = scores
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
