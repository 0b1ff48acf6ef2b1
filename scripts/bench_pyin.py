"""Throughput of the Viterbi-smoothed pitch tracker (ops.pyin) over the 824 seeded synthetic
utterances of 1.5 - 4 s at 16 kHz that the other quality benches use (bench_quality.py), a harmonic
glide added to each so that there is a pitch to find, padded to the longest with `lengths`; prints
one JSON line and writes it to --out (profiles/pyin_bench.json).

    python scripts/bench_pyin.py            # MI355X

One batched call chunked under the default workspace cap, and one with a cap that takes the whole
set at once; one warm-up call each, then --reps timed calls between device events (mean, smallest,
largest), and whether the two give the same bits.  `pitch` is ops.pitch (plain YIN) on the same
batch, timed the same way.  `stages_ms` splits one uncapped call of the first --stage-rows rows
into the d' pass (ops.pitch_stages: YIN's own kernels with d' written out) and the rest (candidates,
Viterbi with its backtrace, output), by difference.  The numpy oracle scripts/pyin_oracle.py is
timed per utterance on the first --cpu utterances on the host, with whether the device's state and
lag equal it on every frame of those.  No time is asserted anywhere.
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
    ap.add_argument('--cpu', type=int, default=2)
    ap.add_argument('--utts', type=int, default=824)
    ap.add_argument('--stage-rows', type=int, default=128)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pyin_bench.json'))
    args = ap.parse_args()
    import torch
    import pyin_oracle
    from bench_quality import utterances
    from segan_pytorch_amd import ops
    rng = np.random.default_rng(1)
    rows = []
    for _, d in utterances(args.utts):
        f0 = np.geomspace(rng.uniform(80, 200), rng.uniform(100, 300), len(d))
        rows.append(d * np.float32(0.3) + np.sin(2 * np.pi * np.cumsum(f0) / 16000).astype(np.float32))
    lengths = [len(d) for d in rows]
    x = torch.zeros(len(rows), max(lengths))
    for i, d in enumerate(rows):
        x[i, :len(d)] = torch.from_numpy(d)
    x = x.cuda()
    per_row = 8 * ops.pyin_dims(1, max(lengths))['ws_doubles']
    whole = per_row * len(rows) + 64
    out = {'leg': 'mi355x', 'op': 'pyin', 'utts': len(rows),
           'mean_audio_s': float(np.mean(lengths)) / 16000, 'reps': args.reps,
           'frames': ops.pyin_dims(1, max(lengths))['frames'],
           'ws_cap_bytes': ops.PYIN_WS_CAP, 'ws_bytes_per_row': per_row,
           'calls_under_cap': -(-len(rows) // max(1, ops.PYIN_WS_CAP // per_row)),
           'one_call_ws_bytes': whole, 'oracle_cpu_utts': args.cpu}
    got, ms = timed(torch, lambda: ops.pyin(x, lengths=lengths), args.reps)
    got1, ms1 = timed(torch, lambda: ops.pyin(x, lengths=lengths, ws_cap=whole), args.reps)
    out['chunked'] = spread(ms, len(rows))
    out['one_call'] = spread(ms1, len(rows))
    out['same_bits'] = bool(all(torch.equal(a.double().view(torch.int64), b.double().view(torch.int64))
                                for a, b in zip(got, got1)))
    out['voiced_share'] = float((got[1] > 0).sum()) / float(got[3].sum())
    del got1
    _, msy = timed(torch, lambda: ops.pitch(x, lengths=lengths), args.reps)
    out['pitch'] = {'chunked': spread(msy, len(rows))}
    n = min(args.stage_rows, len(rows))
    xs, ls = x[:n].contiguous(), lengths[:n]
    big = 1 << 40
    _, ma = timed(torch, lambda: ops.pyin(xs, lengths=ls, ws_cap=big), args.reps)
    _, mb = timed(torch, lambda: ops.pitch_stages(xs, lengths=ls, ws_cap=big), args.reps)
    out['stages_ms'] = {'rows': n, 'pyin': float(np.mean(ma)), 'pitch_with_cmnd': float(np.mean(mb)),
                        'candidates_viterbi_output': float(np.mean(ma) - np.mean(mb))}
    t0 = time.perf_counter()
    tabs = ops.pyin_tables(16000)
    want = [pyin_oracle.track(d, 16000, tabs=tabs) for d in rows[:args.cpu]]
    out['oracle_cpu_s_per_utt'] = (time.perf_counter() - t0) / max(args.cpu, 1)
    st = ops.pyin_stages(x[:max(args.cpu, 1)].contiguous(), lengths=lengths[:max(args.cpu, 1)])
    out['equals_oracle'] = bool(all(
        np.array_equal(st['state'][i, :len(w['lag'])].cpu().numpy(), w['state']) and
        np.array_equal(st['lag'][i, :len(w['lag'])].cpu().numpy(), w['lag']) and
        np.array_equal(st['f0'][i, :len(w['lag'])].cpu().numpy(), w['f0'])
        for i, w in enumerate(want)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
