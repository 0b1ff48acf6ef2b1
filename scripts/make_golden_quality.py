"""Fixture that pins the speech-quality measures (segan_pytorch_amd/quality.py, ops.wss / ops.llr)
to the REAL reference's segan/utils.py, generated in the build container (it needs the reference
checkout, imported through oracle/ref_harness.py):

    python scripts/make_golden_quality.py  ->  tests/golden/quality.pt

Signals (float32): a seeded resonant AR process with a syllable-like envelope (40 000 samples, not
a multiple of the 120-sample hop) and one white-noise track; the noisy versions are
clean + gain * noise, evaluated in float32 (``degraded()``, restated bit for bit by the tests).
Pairs: AR at 0 / 10 / 20 dB, a 16 384-sample white-noise pair, the AR clean with a 2 000-sample run
of exact zeros, a 400-sample pair (no frame), 40 000 vs 39 950 samples, and one 8 kHz pair (per-frame
WSS / LLR only).  The reference's PESQ is patched to return fixed strings.  Also: int16 clean /
noisy files for the eval_noisy_performance.py case, with the reference's CompositeEval rows.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import ref_harness  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'quality.pt')
PESQ_STRINGS = ('2.500', '3.100', 'error!')
CLI_PESQ = '2.500'


def speech_like(n, srate, seed, resonances=((700., 0.95),)):
    """AR process with complex pole pairs at the given (Hz, radius), driven by white noise, times a
    slow syllable envelope; peak 0.5, float32."""
    rng = np.random.default_rng(seed)
    a = np.array([1.0])
    for f, r in resonances:
        w = 2 * np.pi * f / srate
        a = np.convolve(a, [1.0, -2 * r * np.cos(w), r * r])
    from scipy.signal import lfilter
    x = lfilter([1.0], a, rng.standard_normal(n))
    t = np.arange(n) / srate
    env = 0.15 + 0.85 * np.abs(np.sin(2 * np.pi * 2.7 * t + rng.uniform(0, np.pi))) ** 1.5
    x = x * env
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def gain_for(clean, noise, snr_db):
    return np.float32(np.sqrt(np.sum(clean.astype(np.float64) ** 2) /
                              (np.sum(noise.astype(np.float64) ** 2) * 10 ** (snr_db / 10))))


def degraded(clean, noise, gain):
    """clean + gain * noise, two float32 roundings (the tests restate it with torch)."""
    return (clean + np.float32(gain) * noise).astype(np.float32)


def make_pair(signals, gains, recipe):
    clean = signals[recipe['ref']]
    deg = degraded(clean, signals[recipe['noise']], gains[recipe['gain']])[:recipe['len_deg']]
    ref = clean[:recipe['len_ref']].copy()
    if 'zero_ref' in recipe:
        a, b = recipe['zero_ref']
        ref[a:b] = 0
    return ref, deg


def llr_fp64(U, ref, deg, srate):
    """utils.py:598-657 with the quadratic forms in float64 (of the same float32-rounded R / A)."""
    from scipy.linalg import toeplitz
    win = round(30 * srate / 1000.)
    skip = int(np.floor(win / 4))
    P = 10 if srate < 10000 else 16
    nf = int(len(ref) / skip - win / skip)
    window = 0.5 * (1 - np.cos(2 * np.pi * np.linspace(1, win, win) / (win + 1)))
    out = []
    for f in range(nf):
        c = ref[f * skip:f * skip + win] * window
        p = deg[f * skip:f * skip + win] * window
        Rc, _, Ac = U.lpcoeff(c, P)
        _, _, Ap = U.lpcoeff(p, P)
        T = toeplitz(Rc.astype(np.float64))
        Ac, Ap = Ac.astype(np.float64), Ap.astype(np.float64)
        out.append(np.log((Ap @ T @ Ap) / (Ac @ T @ Ac)))
    return np.array(out)


def main():
    ref_harness.import_reference()
    import segan.utils as U
    np.seterr(all='ignore')
    n = 40000
    clean = speech_like(n, 16000, 11)
    noise = np.random.default_rng(12).standard_normal(n).astype(np.float32)
    wclean = (0.3 * np.random.default_rng(13).standard_normal(16384)).astype(np.float32)
    wnoise = np.random.default_rng(14).standard_normal(16384).astype(np.float32)
    clean8 = speech_like(16000, 8000, 15)
    noise8 = np.random.default_rng(16).standard_normal(16000).astype(np.float32)
    zero_at = (20000, 22000)
    gains = {'snr0': gain_for(clean, noise, 0), 'snr10': gain_for(clean, noise, 10),
             'snr20': gain_for(clean, noise, 20), 'white': gain_for(wclean, wnoise, 5),
             'sr8k': gain_for(clean8, noise8, 10)}
    signals = {'clean': clean, 'noise': noise, 'wclean': wclean, 'wnoise': wnoise,
               'clean8': clean8, 'noise8': noise8}
    # name -> how the pair is made from the stored signals (restated by tests/test_gpu_quality.py)
    recipes = {
        'snr0': dict(ref='clean', noise='noise', gain='snr0', len_ref=n, len_deg=n),
        'snr10': dict(ref='clean', noise='noise', gain='snr10', len_ref=n, len_deg=n),
        'snr20': dict(ref='clean', noise='noise', gain='snr20', len_ref=n, len_deg=n),
        'white': dict(ref='wclean', noise='wnoise', gain='white', len_ref=16384, len_deg=16384),
        'zero_run': dict(ref='clean', noise='noise', gain='snr10', len_ref=n, len_deg=n,
                         zero_ref=zero_at),
        'short': dict(ref='clean', noise='noise', gain='snr10', len_ref=400, len_deg=400),
        'unequal': dict(ref='clean', noise='noise', gain='snr10', len_ref=n, len_deg=39950),
        'sr8k': dict(ref='clean8', noise='noise8', gain='sr8k', len_ref=16000, len_deg=16000,
                     srate=8000),
    }
    pairs = {k: make_pair(signals, gains, v) + (v.get('srate', 16000),) for k, v in recipes.items()}
    results, llr_gap = {}, 0.0
    for name, (r, d, sr) in pairs.items():
        L = min(len(r), len(d))
        rt, dt = r[:L], d[:L]
        res = {'wss': torch.tensor(np.array(U.wss(rt, dt, sr), dtype=np.float64)),
               'llr': torch.tensor(np.asarray(U.llr(rt, dt, sr), dtype=np.float64).reshape(-1)),
               'ssnr': torch.tensor(np.array(U.SSNR(rt, dt, sr)[1], dtype=np.float64))}
        l64 = llr_fp64(U, rt, dt, sr)
        fin = np.isfinite(l64)
        assert np.array_equal(fin, np.isfinite(res['llr'].numpy())), name
        if fin.any():
            llr_gap = max(llr_gap, float(np.abs(l64[fin] - res['llr'].numpy()[fin]).max()))
        if sr == 16000:
            comp = {}
            for s in PESQ_STRINGS:
                U.PESQ = lambda a, b, s=s: s
                comp[s] = torch.tensor(np.array(U.CompositeEval(r, d, True), dtype=np.float64))
            res['composite'] = comp
        results[name] = res
    zc = results['zero_run']['composite']['2.500']
    assert np.isnan(zc[0]) and np.isfinite(zc[1]) and np.isnan(zc[2]), zc

    # eval_noisy_performance.py: int16 files; rows of CompositeEval on x / 32768 (float32)
    U.PESQ = lambda a, b: CLI_PESQ
    cli = {'names': [], 'clean': [], 'noisy': [], 'rows': []}
    fmt = '{:.3f} {:.3f} {:.3f} {:.3f} {:.3}'
    seed = 40
    for i, L in enumerate((12000, 14401, 17003)):
        while True:   # keep every printed figure well away from a rounding boundary
            seed += 1
            c16 = np.round(speech_like(L, 16000, seed) * 32767).astype(np.int16)
            nz = np.random.default_rng(seed + 1000).standard_normal(L) * 1500
            n16 = np.clip(np.round(c16 + nz), -32768, 32767).astype(np.int16)
            row = U.CompositeEval(c16.astype(np.float32) / 32768, n16.astype(np.float32) / 32768, True)
            v = np.array(row, dtype=np.float64)
            q = [v[0] * 1e3, v[1] * 1e3, v[2] * 1e3, v[3] * 1e3,
                 v[4] * 10 ** (3 - 1 - np.floor(np.log10(abs(v[4]))))]
            if all(abs(x - np.floor(x) - 0.5) > 0.05 for x in q):
                break
        cli['names'].append('utt{}.wav'.format(i))
        cli['clean'].append(torch.from_numpy(c16))
        cli['noisy'].append(torch.from_numpy(n16))
        cli['rows'].append(torch.tensor(v))
    cli['pesq'] = CLI_PESQ
    cli['format'] = fmt

    fx = {
        'signals': {k: torch.from_numpy(v) for k, v in signals.items()},
        'gains': {k: float(v) for k, v in gains.items()},
        'recipes': recipes,
        'results': results,
        'pesq_strings': PESQ_STRINGS,
        'cli': cli,
        'meta': {'llr_fp32_vs_fp64_max_abs': llr_gap, 'numpy': np.__version__,
                 'alpha': 0.95},
    }
    torch.save(fx, OUT)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes; llr fp32-vs-fp64 gap', llr_gap)


if __name__ == '__main__':
    main()
