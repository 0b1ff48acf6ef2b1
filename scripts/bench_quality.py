"""Evaluation rate of quality.composite_eval (WSS + LLR + segmental SNR, no PESQ) over 824 seeded
synthetic utterances of 1.5 - 4 s at 16 kHz (the size of the VCTK test set), one call per
utterance like eval_noisy_performance.py, with a device synchronise; prints one JSON line.

    python scripts/bench_quality.py            # MI355X
    python scripts/bench_quality.py --cpu-ref N  # the reference's numpy CompositeEval on N of the
                                                 # same utterances (needs the reference checkout)
    python scripts/bench_quality.py --measures   # and, in the same run, ONE batched call each of
        # quality.fwsegsnr / cepstral_distance / si_sdr over the set padded to its longest
        # utterance with `lengths`, beside quality.stoi's batched call; the JSON line also goes to
        # --out (profiles/measures_bench.json)
    python scripts/bench_quality.py --sdr        # instead: ONE batched call of quality.sdr (BSS-eval
        # SDR, 512 taps) over the same set, and the numpy oracle scripts/sdr_oracle.py on
        # --sdr-cpu of its utterances; the JSON line also goes to --sdr-out
        # (profiles/sdr_bench.json)
    python scripts/bench_quality.py --srmr       # instead: ONE call of quality.srmr over the degraded
        # signals of the same set (ops.srmr chunks it under its workspace cap), and the numpy /
        # scipy oracle scripts/srmr_oracle.py on --srmr-cpu of its utterances; the JSON line also
        # goes to --srmr-out (profiles/srmr_bench.json)
    python scripts/bench_quality.py --pitch      # instead: ONE call each of quality.pitch over the
        # degraded signals and of quality.f0_eval (two trackings and the measures) over the same
        # set with a harmonic glide added to every utterance, and the numpy oracle
        # scripts/pitch_oracle.py on --pitch-cpu of its utterances; the JSON line also goes to
        # --pitch-out (profiles/pitch_bench.json)
"""
import argparse
import ctypes
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
    ap.add_argument('--measures', action='store_true',
                    help='also time the batched fwSNRseg + CD + SI-SDR call (and STOI\'s)')
    ap.add_argument('--batch-reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'measures_bench.json'))
    ap.add_argument('--sdr', action='store_true',
                    help='time the batched BSS-eval SDR call and its numpy oracle instead')
    ap.add_argument('--sdr-cpu', type=int, default=3)
    ap.add_argument('--sdr-out', default=os.path.join(ROOT, 'profiles', 'sdr_bench.json'))
    ap.add_argument('--srmr', action='store_true',
                    help='time the batched SRMR call and its numpy / scipy oracle instead')
    ap.add_argument('--srmr-cpu', type=int, default=3)
    ap.add_argument('--srmr-out', default=os.path.join(ROOT, 'profiles', 'srmr_bench.json'))
    ap.add_argument('--pitch', action='store_true',
                    help='time the batched pitch tracking and F0 measures and their numpy oracle '
                         'instead')
    ap.add_argument('--pitch-cpu', type=int, default=3)
    ap.add_argument('--pitch-out', default=os.path.join(ROOT, 'profiles', 'pitch_bench.json'))
    args = ap.parse_args()
    utts = utterances()
    if args.pitch:
        import torch
        out = batched_pitch(torch, utts, args.batch_reps, args.pitch_cpu)
        with open(args.pitch_out, 'w') as f:
            f.write(json.dumps(out) + '\n')
        print(json.dumps(out))
        return
    if args.srmr:
        import torch
        out = batched_srmr(torch, utts, args.batch_reps, args.srmr_cpu)
        with open(args.srmr_out, 'w') as f:
            f.write(json.dumps(out) + '\n')
        print(json.dumps(out))
        return
    if args.sdr:
        import torch
        out = batched_sdr(torch, utts, args.batch_reps, args.sdr_cpu)
        with open(args.sdr_out, 'w') as f:
            f.write(json.dumps(out) + '\n')
        print(json.dumps(out))
        return
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
    out = {'leg': 'mi355x', 'utts': len(dev), 'seconds': dt, 'utts_per_s': len(dev) / dt,
           'mean_s_per_utt': dt / len(dev),
           'mean_audio_s': float(np.mean([len(c) for c, _ in utts])) / 16000,
           'last_csig': float(r['csig'][0])}
    if args.measures:
        out['measures'] = batched_measures(torch, utts, args.batch_reps)
        with open(args.out, 'w') as f:
            f.write(json.dumps(out) + '\n')
    print(json.dumps(out))


def batched_measures(torch, utts, reps):
    """Seconds of one batched call (after one warm-up call, mean of `reps`, up to a device
    synchronise) of the three measures together, of each alone, and of quality.stoi."""
    from segan_pytorch_amd import quality
    lengths = [len(c) for c, _ in utts]
    ref = torch.zeros(len(utts), max(lengths))
    deg = torch.zeros(len(utts), max(lengths))
    for i, (c, d) in enumerate(utts):
        ref[i, :len(c)] = torch.from_numpy(c)
        deg[i, :len(d)] = torch.from_numpy(d)
    ref, deg = ref.cuda(), deg.cuda()

    def timed(fn):
        res = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            res = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, res

    legs = {'fwsegsnr': lambda: quality.fwsegsnr(ref, deg, lengths=lengths),
            'cd': lambda: quality.cepstral_distance(ref, deg, lengths=lengths),
            'sisdr': lambda: quality.si_sdr(ref, deg, lengths=lengths)}
    out = {}
    dt, res = timed(lambda: [fn() for fn in legs.values()])
    out['batched_seconds'] = dt
    out['batched_utts_per_s'] = len(utts) / dt
    for (k, fn), v in zip(legs.items(), res):
        out[k + '_seconds'] = timed(fn)[0]
        out['mean_' + k] = float(v[torch.isfinite(v)].mean())
        out[k + '_nonfinite_rows'] = int((~torch.isfinite(v)).sum())
    out['stoi_batched_seconds'] = timed(lambda: quality.stoi(ref, deg, lengths=lengths))[0]
    return out


def batched_sdr(torch, utts, reps, ncpu):
    """Seconds of one batched quality.sdr call over the whole set (after one warm-up call, mean of
    `reps`, up to a device synchronise), the oracle's seconds per utterance on the first `ncpu`
    utterances, and the largest difference between the two on those."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import sdr_oracle
    from segan_pytorch_amd import ops, quality
    lengths = [len(c) for c, _ in utts]
    ref = torch.zeros(len(utts), max(lengths))
    deg = torch.zeros(len(utts), max(lengths))
    for i, (c, d) in enumerate(utts):
        ref[i, :len(c)] = torch.from_numpy(c)
        deg[i, :len(d)] = torch.from_numpy(d)
    ref, deg = ref.cuda(), deg.cuda()
    v = quality.sdr(ref, deg, lengths=lengths)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        v = quality.sdr(ref, deg, lengths=lengths)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    t0 = time.perf_counter()
    want = [sdr_oracle.sdr(c, d) for c, d in utts[:ncpu]]
    cpu = (time.perf_counter() - t0) / max(ncpu, 1)
    got = v[:ncpu].cpu().tolist()
    return {'leg': 'mi355x', 'measure': 'sdr', 'taps': ops.SDR_TAPS, 'utts': len(utts),
            'mean_audio_s': float(np.mean(lengths)) / 16000, 'batched_seconds': dt,
            'batched_utts_per_s': len(utts) / dt, 'mean_sdr': float(v[torch.isfinite(v)].mean()),
            'sdr_nonfinite_rows': int((~torch.isfinite(v)).sum()),
            'oracle_cpu_utts': ncpu, 'oracle_cpu_s_per_utt': cpu,
            'max_abs_diff_db_vs_oracle': max([abs(a - b) for a, b in zip(got, want)] or [0.0])}


def batched_srmr(torch, utts, reps, ncpu):
    """Seconds of one quality.srmr call over the degraded signals of the whole set (after one
    warm-up call, mean of `reps`, up to a device synchronise; ops.srmr walks the rows in chunks
    under its workspace cap), the oracle's seconds per utterance on the first `ncpu` utterances,
    and the largest relative difference between the two on those."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import srmr_oracle
    from segan_pytorch_amd import _lib, ops, quality
    lengths = [len(d) for _, d in utts]
    deg = torch.zeros(len(utts), max(lengths))
    for i, (_, d) in enumerate(utts):
        deg[i, :len(d)] = torch.from_numpy(d)
    deg = deg.cuda()
    v = quality.srmr(deg, lengths=lengths)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        v = quality.srmr(deg, lengths=lengths)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    dims = (ctypes.c_int64 * 4)()
    _lib.load().segan_srmr_dims(len(utts), max(lengths), 16000, dims)
    # the same with a cap that takes the whole set in one call of segan_srmr
    whole = 8 * dims[3] + 64
    one = ops.srmr(deg, lengths=lengths, ws_cap=whole)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        one = ops.srmr(deg, lengths=lengths, ws_cap=whole)
    torch.cuda.synchronize()
    dt_one = (time.perf_counter() - t0) / reps
    same = bool(torch.equal(one.view(torch.int64), v.view(torch.int64)))
    t0 = time.perf_counter()
    want = [srmr_oracle.srmr(d) for _, d in utts[:ncpu]]
    cpu = (time.perf_counter() - t0) / max(ncpu, 1)
    got = v[:ncpu].cpu().tolist()
    return {'leg': 'mi355x', 'measure': 'srmr', 'utts': len(utts),
            'mean_audio_s': float(np.mean(lengths)) / 16000, 'batched_seconds': dt,
            'batched_utts_per_s': len(utts) / dt, 'mean_srmr': float(v[torch.isfinite(v)].mean()),
            'srmr_nonfinite_rows': int((~torch.isfinite(v)).sum()),
            'ws_cap_bytes': ops.SRMR_WS_CAP, 'ws_bytes_per_row': 8 * dims[2],
            'calls': -(-len(utts) // max(1, ops.SRMR_WS_CAP // (8 * dims[2]))),
            'one_call_ws_bytes': whole, 'one_call_seconds': dt_one,
            'one_call_utts_per_s': len(utts) / dt_one, 'one_call_same_bits': same,
            'oracle_cpu_utts': ncpu, 'oracle_cpu_s_per_utt': cpu,
            'max_rel_diff_vs_oracle': max([abs(a - b) / abs(b) for a, b in zip(got, want)]
                                          or [0.0])}


def batched_pitch(torch, utts, reps, ncpu):
    """Seconds of one quality.pitch call over the degraded signals of the whole set and of one
    quality.f0_eval call over the pairs (after one warm-up call each, mean of `reps`, up to a
    device synchronise; ops.pitch walks the rows in chunks under its workspace cap), with a
    harmonic glide added to every utterance so that there is a pitch to find; the oracle's seconds
    per utterance (two trackings and the measures) on the first `ncpu` utterances, whether every
    lag agrees on those, and the largest difference in f0_mae."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    import pitch_oracle
    from segan_pytorch_amd import ops, quality
    rng = np.random.default_rng(1)
    pairs = []
    for c, d in utts:
        f0 = np.geomspace(rng.uniform(80, 200), rng.uniform(100, 300), len(c))
        h = np.sin(2 * np.pi * np.cumsum(f0) / 16000).astype(np.float32)
        pairs.append((c * np.float32(0.1) + h, d * np.float32(0.3) + h))
    lengths = [len(c) for c, _ in pairs]
    ref = torch.zeros(len(pairs), max(lengths))
    deg = torch.zeros(len(pairs), max(lengths))
    for i, (c, d) in enumerate(pairs):
        ref[i, :len(c)] = torch.from_numpy(c)
        deg[i, :len(d)] = torch.from_numpy(d)
    ref, deg = ref.cuda(), deg.cuda()

    def timed(fn):
        out = fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) / reps

    (f0, voiced, _), dt_pitch = timed(lambda: quality.pitch(deg, lengths=lengths))
    ev, dt_eval = timed(lambda: quality.f0_eval(ref, deg, lengths=lengths))
    per_row = 8 * ops.pitch_dims(1, max(lengths))['ws_doubles']
    t0 = time.perf_counter()
    want = [(pitch_oracle.track(c), pitch_oracle.track(d)) for c, d in pairs[:ncpu]]
    want_ev = [pitch_oracle.f0_eval(a['f0'], a['lag'], b['f0'], b['lag']) for a, b in want]
    cpu = (time.perf_counter() - t0) / max(ncpu, 1)
    same = all(np.array_equal(b['lag'] > 0, voiced[i, :len(b['lag'])].cpu().numpy())
               for i, (_, b) in enumerate(want))
    mae = ev['f0_mae']
    return {'leg': 'mi355x', 'measure': 'pitch', 'utts': len(pairs),
            'mean_audio_s': float(np.mean(lengths)) / 16000, 'frames': int(f0.shape[1]),
            'pitch_seconds': dt_pitch, 'pitch_utts_per_s': len(pairs) / dt_pitch,
            'f0_eval_seconds': dt_eval, 'f0_eval_utts_per_s': len(pairs) / dt_eval,
            'ws_cap_bytes': ops.PITCH_WS_CAP, 'ws_bytes_per_row': per_row,
            'calls': -(-len(pairs) // max(1, ops.PITCH_WS_CAP // per_row)),
            'mean_voiced_share': float(ev['voiced'].mean()),
            'mean_f0_mae': float(mae[torch.isfinite(mae)].mean()),
            'f0_mae_nonfinite_rows': int((~torch.isfinite(mae)).sum()),
            'mean_vuv_acc': float(ev['vuv_acc'].mean()),
            'oracle_cpu_utts': ncpu, 'oracle_cpu_s_per_utt_pair': cpu,
            'voicing_same_as_oracle': bool(same),
            'max_abs_diff_f0_mae_vs_oracle': max(
                [abs(float(mae[i]) - float(w['f0_mae'])) for i, w in enumerate(want_ev)] or [0.0])}


if __name__ == '__main__':
    main()
