"""Throughput of the OM-LSA enhancer with IMCRA noise tracking (ops.omlsa_rows) over the 824 seeded
synthetic utterances of 1.5 - 4 s at 16 kHz that bench_denoise.py runs (bench_quality.py), padded
to the longest with `lengths`, with log-MMSE (ops.denoise_rows) timed in the same run for
comparison; prints one JSON line and writes it to --out (profiles/omlsa_bench.json).

    python scripts/bench_omlsa.py            # MI355X

Per enhancer: one call chunked under the default workspace cap, and one call with a cap that takes
the whole set at once; one warm-up call each, then --reps timed calls between device events (mean,
smallest, largest), and whether the two give the same bits.  The numpy oracle
scripts/omlsa_oracle.py is timed per utterance on the first --cpu utterances on the host, with its
largest distance from the device's result on those.  `fixture` holds, for the four long rows of
tests/golden/omlsa.pt (noise whose level is flat, steps up, steps down, ramps), the SNR over the
voiced samples after 2.5 s of the noisy row and of wiener, logmmse and omlsa on the device.
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
    ap.add_argument('--cpu', type=int, default=3)
    ap.add_argument('--utts', type=int, default=824)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'omlsa_bench.json'))
    args = ap.parse_args()
    import torch
    import make_golden_omlsa as GO
    import omlsa_oracle
    from bench_denoise import spread, timed
    from bench_quality import utterances
    from segan_pytorch_amd import ops
    utts = utterances(args.utts)
    lengths = [len(d) for _, d in utts]
    deg = torch.zeros(len(utts), max(lengths))
    for i, (_, d) in enumerate(utts):
        deg[i, :len(d)] = torch.from_numpy(d)
    deg = deg.cuda()
    out = {'leg': 'mi355x', 'op': 'omlsa_rows', 'utts': len(utts),
           'mean_audio_s': float(np.mean(lengths)) / 16000, 'reps': args.reps,
           'oracle_cpu_utts': args.cpu}
    legs = (('omlsa', ops.omlsa_dims, ops.OMLSA_WS_CAP,
             lambda **kw: ops.omlsa_rows(deg, lengths=lengths, out_dtype=torch.float64, **kw)),
            ('logmmse', ops.denoise_dims, ops.DENOISE_WS_CAP,
             lambda **kw: ops.denoise_rows(deg, lengths=lengths, rule='logmmse',
                                           out_dtype=torch.float64, **kw)))
    for name, dims, cap, fn in legs:
        per_row = dims(1, max(lengths))['ws_bytes']
        whole = per_row * len(utts) + 64
        y, ms = timed(torch, fn, args.reps)
        y1, ms1 = timed(torch, lambda: fn(ws_cap=whole), args.reps)
        out[name] = {'ws_cap_bytes': cap, 'ws_bytes_per_row': per_row,
                     'calls_under_cap': -(-len(utts) // max(1, cap // per_row)),
                     'one_call_ws_bytes': whole, 'chunked': spread(ms, len(utts)),
                     'one_call': spread(ms1, len(utts)),
                     'same_bits': bool(torch.equal(y.view(torch.int64), y1.view(torch.int64)))}
        if name == 'omlsa':
            t0 = time.perf_counter()
            want = [omlsa_oracle.omlsa(d, 16000)['y'] for _, d in utts[:args.cpu]]
            out[name]['oracle_cpu_s_per_utt'] = (time.perf_counter() - t0) / max(args.cpu, 1)
            out[name]['max_diff_vs_oracle_rel_peak'] = max(
                [float(np.abs(y[i, :len(w)].cpu().numpy() - w).max() / np.abs(utts[i][1]).max())
                 for i, w in enumerate(want)] or [0.0])
    fx = torch.load(os.path.join(ROOT, 'tests', 'golden', 'omlsa.pt'), map_location='cpu',
                    weights_only=False)
    sig = {k: v.numpy() for k, v in fx['signals'].items()}
    _, active = GO.gated6()
    scores = {}
    for kind, x in GO.long_rows(sig, fx['gains']).items():
        xd = torch.from_numpy(x).cuda()
        scores[kind] = {name: GO.late_snr(sig['clean4'], y.cpu().numpy(), active) for name, y in (
            ('noisy', xd), ('wiener', ops.denoise_rows(xd, rule='wiener')),
            ('logmmse', ops.denoise_rows(xd, rule='logmmse')), ('omlsa', ops.omlsa_rows(xd)))}
    out['fixture_late_snr_db'] = scores
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
