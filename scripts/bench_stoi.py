"""Evaluation rate of quality.stoi over 824 seeded synthetic utterances of 1.5 - 4 s at 16 kHz with
pauses (the size of the VCTK test set), in two modes, each after a warm-up and timed up to a
device synchronise: one call per utterance (as eval_noisy_performance.py --stoi does), and one
batched call over the set padded to its longest utterance with `lengths`.  Prints one JSON line.

    python scripts/bench_stoi.py                 # MI355X
    python scripts/bench_stoi.py --estoi         # and quality.estoi next to it, under 'estoi'
    python scripts/bench_stoi.py --cpu-oracle N  # the fp64 numpy oracle (scripts/stoi_oracle.py)
                                                 # on N of the same utterances, on the CPU
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def utterances(n=824, seed=0):
    """Noise bursts under a 1.5 Hz half-wave envelope (the other half 80 dB down: pauses the
    silent-frame removal drops), and the same plus white noise of standard deviation 0.3."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.uniform(1.5, 4.0) * 16000)
        t = np.arange(L) / 16000
        c = rng.standard_normal(L) * np.maximum(np.sin(2 * np.pi * 1.5 * t + rng.uniform(0, 6)),
                                                1e-4)
        d = c + 0.3 * rng.standard_normal(L)
        out.append((c.astype(np.float32), d.astype(np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cpu-oracle', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch-reps', type=int, default=5)
    ap.add_argument('--estoi', action='store_true',
                    help='time quality.estoi the same two ways after STOI, in the same run')
    args = ap.parse_args()
    utts = utterances()
    audio_s = float(np.sum([len(c) for c, _ in utts])) / 16000
    if args.cpu_oracle:
        sys.path.insert(0, os.path.join(ROOT, 'scripts'))
        import stoi_oracle
        t0 = time.perf_counter()
        for c, d in utts[:args.cpu_oracle]:
            stoi_oracle.stoi(c, d, 16000)
        dt = time.perf_counter() - t0
        print(json.dumps({'leg': 'numpy_oracle_cpu', 'utts': args.cpu_oracle,
                          'mean_s_per_utt': dt / args.cpu_oracle,
                          'mean_audio_s': float(np.mean([len(c) for c, _ in
                                                         utts[:args.cpu_oracle]])) / 16000}))
        return
    import torch
    from segan_pytorch_amd import quality
    dev = [(torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda()) for c, d in utts]
    T = max(len(c) for c, _ in utts)
    ref = torch.zeros(len(utts), T)
    deg = torch.zeros(len(utts), T)
    for i, (c, d) in enumerate(utts):
        ref[i, :len(c)] = torch.from_numpy(c)
        deg[i, :len(d)] = torch.from_numpy(d)
    ref, deg = ref.cuda(), deg.cuda()
    lengths = [len(c) for c, _ in utts]

    def measure(fn):
        for c, d in dev[:args.warmup]:
            fn(c, d)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per = [fn(c, d) for c, d in dev]
        torch.cuda.synchronize()
        dt_single = time.perf_counter() - t0
        per = torch.cat(per)
        fn(ref, deg, lengths=lengths)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.batch_reps):
            batched = fn(ref, deg, lengths=lengths)
        torch.cuda.synchronize()
        dt_batch = (time.perf_counter() - t0) / args.batch_reps
        same = bool(torch.equal(batched.cpu().view(torch.int64), per.cpu().view(torch.int64)))
        return {'per_utt_seconds': dt_single, 'per_utt_utts_per_s': len(utts) / dt_single,
                'batched_seconds': dt_batch, 'batched_utts_per_s': len(utts) / dt_batch,
                'batched_equals_per_utt_bitwise': same,
                'nan_rows': int(torch.isnan(per).sum()),
                'mean': float(per[~torch.isnan(per)].mean())}

    out = {'leg': 'mi355x', 'utts': len(utts), 'audio_s': audio_s}
    r = measure(quality.stoi)
    out['mean_stoi'] = r.pop('mean')
    out.update(r)
    if args.estoi:
        r = measure(quality.estoi)
        r['mean_estoi'] = r.pop('mean')
        r['batched_seconds_over_stois'] = r['batched_seconds'] / out['batched_seconds']
        out['estoi'] = r
    print(json.dumps(out))


if __name__ == '__main__':
    main()
