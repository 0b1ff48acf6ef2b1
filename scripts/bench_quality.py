"""Evaluation rate of quality.composite_eval (WSS + LLR + segmental SNR, no PESQ) over 824 seeded
synthetic utterances of 1.5 - 4 s at 16 kHz (the size of the VCTK test set), one call per
utterance like eval_noisy_performance.py, with a device synchronise; prints one JSON line.

    python scripts/bench_quality.py            # MI355X
    python scripts/bench_quality.py --cpu-ref N  # the reference's numpy CompositeEval on N of the
                                                 # same utterances (needs the reference checkout)
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
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.uniform(1.5, 4.0) * 16000)
        t = np.arange(L) / 16000
        c = rng.standard_normal(L) * np.abs(np.sin(2 * np.pi * 3 * t))
        d = c + 0.3 * rng.standard_normal(L)
        out.append((c.astype(np.float32), d.astype(np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cpu-ref', type=int, default=0)
    ap.add_argument('--warmup', type=int, default=20)
    args = ap.parse_args()
    utts = utterances()
    if args.cpu_ref:
        sys.path.insert(0, os.path.join(ROOT, 'oracle'))
        import ref_harness
        ref_harness.import_reference()
        import segan.utils as U
        U.PESQ = lambda a, b: '2.500'
        t0 = time.perf_counter()
        for c, d in utts[:args.cpu_ref]:
            U.CompositeEval(c, d, True)
        dt = time.perf_counter() - t0
        print(json.dumps({'leg': 'reference_cpu', 'utts': args.cpu_ref,
                          'mean_s_per_utt': dt / args.cpu_ref,
                          'mean_audio_s': float(np.mean([len(c) for c, _ in utts[:args.cpu_ref]])) / 16000}))
        return
    import torch
    from segan_pytorch_amd.quality import composite_eval
    dev = [(torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda()) for c, d in utts]
    for c, d in dev[:args.warmup]:
        composite_eval(c, d, pesq=2.5)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c, d in dev:
        r = composite_eval(c, d, pesq=2.5)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({'leg': 'mi355x', 'utts': len(dev), 'seconds': dt, 'utts_per_s': len(dev) / dt,
                      'mean_s_per_utt': dt / len(dev),
                      'mean_audio_s': float(np.mean([len(c) for c, _ in utts])) / 16000,
                      'last_csig': float(r['csig'][0])}))


if __name__ == '__main__':
    main()
