"""Throughput of the Wiener / log-MMSE baseline enhancers (ops.denoise_rows) over the 824 seeded
synthetic utterances of 1.5 - 4 s at 16 kHz that the other quality benches use (bench_quality.py),
padded to the longest with `lengths`; prints one JSON line and writes it to --out
(profiles/denoise_bench.json).

    python scripts/bench_denoise.py            # MI355X

Per rule: one call chunked under the default workspace cap, and one call with a cap that takes the
whole set at once; one warm-up call each, then --reps timed calls between device events (mean,
smallest, largest), and whether the two give the same bits.  The numpy oracle
scripts/denoise_oracle.py is timed per utterance on the first --cpu utterances on the host, with
its largest distance from the device's result on those.  `fixture` holds SI-SDR and fwSNRseg
(quality.si_sdr / quality.fwsegsnr) of the fixture's noisy signal and of both baselines against its
clean signal.
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


def timed(torch, fn, reps):
    """(result, [milliseconds of each of `reps` calls between device events]) after one warm-up"""
    out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, ms


def spread(ms, n):
    return {'mean_ms': float(np.mean(ms)), 'min_ms': float(np.min(ms)), 'max_ms': float(np.max(ms)),
            'utts_per_s': n / (float(np.mean(ms)) / 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu', type=int, default=3)
    ap.add_argument('--utts', type=int, default=824)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'denoise_bench.json'))
    args = ap.parse_args()
    import torch
    import denoise_oracle
    from bench_quality import utterances
    from segan_pytorch_amd import ops, quality
    utts = utterances(args.utts)
    lengths = [len(d) for _, d in utts]
    deg = torch.zeros(len(utts), max(lengths))
    for i, (_, d) in enumerate(utts):
        deg[i, :len(d)] = torch.from_numpy(d)
    deg = deg.cuda()
    per_row = ops.denoise_dims(1, max(lengths))['ws_bytes']
    whole = per_row * len(utts) + 64
    out = {'leg': 'mi355x', 'op': 'denoise_rows', 'utts': len(utts),
           'mean_audio_s': float(np.mean(lengths)) / 16000, 'reps': args.reps,
           'ws_cap_bytes': ops.DENOISE_WS_CAP, 'ws_bytes_per_row': per_row,
           'calls_under_cap': -(-len(utts) // max(1, ops.DENOISE_WS_CAP // per_row)),
           'one_call_ws_bytes': whole, 'oracle_cpu_utts': args.cpu}
    for rule in sorted(ops.DENOISE_RULES):
        y, ms = timed(torch, lambda: ops.denoise_rows(deg, lengths=lengths, rule=rule,
                                                      out_dtype=torch.float64), args.reps)
        y1, ms1 = timed(torch, lambda: ops.denoise_rows(deg, lengths=lengths, rule=rule,
                                                        out_dtype=torch.float64, ws_cap=whole),
                        args.reps)
        leg = {'chunked': spread(ms, len(utts)), 'one_call': spread(ms1, len(utts)),
               'same_bits': bool(torch.equal(y.view(torch.int64), y1.view(torch.int64)))}
        t0 = time.perf_counter()
        want = [denoise_oracle.denoise(d, 16000, rule)['y'] for _, d in utts[:args.cpu]]
        leg['oracle_cpu_s_per_utt'] = (time.perf_counter() - t0) / max(args.cpu, 1)
        leg['max_diff_vs_oracle_rel_peak'] = max(
            [float(np.abs(y[i, :len(w)].cpu().numpy() - w).max() / np.abs(utts[i][1]).max())
             for i, w in enumerate(want)] or [0.0])
        out[rule] = leg
    fx = torch.load(os.path.join(ROOT, 'tests', 'golden', 'denoise.pt'), map_location='cpu',
                    weights_only=False)
    clean, noisy = fx['signals']['clean'].cuda(), fx['signals']['noisy'].cuda()
    scores = {}
    for name, sig in (('noisy', noisy), ('wiener', ops.denoise_rows(noisy, rule='wiener')),
                      ('logmmse', ops.denoise_rows(noisy, rule='logmmse'))):
        scores[name] = {'si_sdr_db': float(quality.si_sdr(clean, sig)[0]),
                        'fwsegsnr_db': float(quality.fwsegsnr(clean, sig)[0])}
    out['fixture'] = scores
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
