"""Writes tests/golden/stoi.pt: the STOI fixture of ops.stoi / quality.stoi, computed with the fp64
numpy oracle scripts/stoi_oracle.py.

    python scripts/make_golden_stoi.py [out.pt]

Signals (seeded): a 3 s AR "speech" track at 16 kHz whose envelope has pauses 80 dB down (so the
silent-frame removal drops frames) and a white-noise track, both stored as int16 (x / 32768 is
the float32 signal).  Each case is a slice of them, rebuilt by `case_signals`.  Stored: the plan
(taps, band edges) of every rate used, d of every case, every intermediate of two cases, and three
int16 wav pairs for the eval CLI with their d.  The recipe asserts that the closed-form resampling
equals the upfirdn procedure, that no keep / drop decision lies within 1e-6 dB of the threshold,
that an all-zero processed window occurs (the NaN-ignoring minimum), and that d is strictly
monotone in the SNR.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import stoi_oracle as S  # noqa: E402

SR = 16000
LEN = 3 * SR
SNRS = (-5, 0, 10, 20)
STAGE_CASES = ('stage16k', 'stage8k')


def speech(rng, n, sr=SR):
    """AR(2) resonance near 500 Hz plus a spectral tilt, gated by syllables of 150-400 ms and
    pauses of 80-250 ms at -80 dB with 20 ms raised-cosine ramps; peak 0.5."""
    from scipy.signal import lfilter
    r, f0 = 0.97, 500.0
    s = lfilter([1.0], [1.0, -2 * r * math.cos(2 * math.pi * f0 / sr), r * r],
                rng.standard_normal(n))
    s = lfilter([1.0, -0.5], [1.0], s)
    env = np.full(n, 1e-4)
    ramp = int(0.02 * sr)
    t = int(rng.uniform(0.05, 0.15) * sr)
    while t < n:
        on = int(rng.uniform(0.15, 0.4) * sr)
        seg = np.ones(on)
        seg[:ramp] = 0.5 - 0.5 * np.cos(np.pi * np.arange(ramp) / ramp)
        seg[-ramp:] = seg[:ramp][::-1]
        seg = np.maximum(seg * rng.uniform(0.3, 1.0), 1e-4)
        env[t:t + on] = seg[:n - t]
        t += on + int(rng.uniform(0.08, 0.25) * sr)
    x = s * env
    return 0.5 * x / np.abs(x).max()


def to_int16(x):
    return np.clip(np.rint(np.asarray(x) * 32768), -32768, 32767).astype(np.int16)


def to_float(x16):
    return np.asarray(x16).astype(np.float32) / np.float32(32768)


def case_signals(fx, name):
    """(ref, deg, srate) of fixture case `name` as float32 numpy arrays: a slice [start,
    start+len) of the stored clean track; deg = clean + gain * noise (float32), or scale * clean;
    deg zeroed over zero_deg; ref zeroed with silent_ref."""
    rc = fx['cases'][name]
    a, L = rc['start'], rc['len']
    clean = to_float(fx['signals']['clean'])[a:a + L].copy()
    noise = to_float(fx['signals']['noise'])[a:a + L]
    if 'scale' in rc:
        deg = (clean * np.float32(rc['scale'])).astype(np.float32)
    else:
        deg = (clean + np.float32(rc['gain']) * noise).astype(np.float32)
    if 'zero_deg' in rc:
        deg[rc['zero_deg'][0]:rc['zero_deg'][1]] = 0
    if rc.get('silent_ref'):
        clean[:] = 0
    return clean, deg, rc['srate']


def threshold_margin(E):
    """Smallest |E - max + 40| over the finite frame energies (dB)."""
    fin = np.isfinite(E)
    if not fin.any():
        return math.inf
    return float(np.min(np.abs(E[fin] - np.max(E) + S.DYN)))


def main(out):
    import torch
    rng = np.random.default_rng(20251016)
    clean16 = to_int16(speech(rng, LEN))
    noise16 = to_int16(0.1 * rng.standard_normal(LEN))
    c, n = to_float(clean16).astype(np.float64), to_float(noise16).astype(np.float64)

    def gain(snr, a=0, L=LEN):
        return float(np.float32(math.sqrt(np.sum(c[a:a + L] ** 2) / np.sum(n[a:a + L] ** 2) /
                                          10 ** (snr / 10))))

    cases = {}
    for snr in SNRS:
        cases['snr{}'.format(snr).replace('-', 'm')] = dict(srate=SR, start=0, len=LEN,
                                                            gain=gain(snr))
    cases['scaled'] = dict(srate=SR, start=0, len=LEN, scale=0.25)
    cases['zero_run'] = dict(srate=SR, start=0, len=LEN, gain=gain(10),
                             zero_deg=(int(0.8 * SR), int(2.3 * SR)))
    cases['short'] = dict(srate=SR, start=0, len=SR // 4, gain=gain(10))
    cases['silent'] = dict(srate=SR, start=0, len=SR, gain=gain(10), silent_ref=True)
    cases['sr10k'] = dict(srate=10000, start=0, len=30000, gain=gain(0))
    cases['sr8k'] = dict(srate=8000, start=0, len=24000, gain=gain(10))
    cases['sr44k'] = dict(srate=44100, start=0, len=44100, gain=gain(10))
    cases['odd_len'] = dict(srate=SR, start=0, len=LEN - 3, gain=gain(10))
    cases['stage16k'] = dict(srate=SR, start=SR // 2, len=SR, gain=gain(0))
    cases['stage8k'] = dict(srate=8000, start=24000, len=8000, gain=gain(10))
    assert (LEN - 3) * 5 % 8 != 0

    fx = {'signals': {'clean': torch.from_numpy(clean16), 'noise': torch.from_numpy(noise16)},
          'cases': cases}

    plans = {}
    for sr in sorted({rc['srate'] for rc in cases.values()}):
        p, q, taps = S.plan(sr)
        plans[sr] = {'p': p, 'q': q, 'taps': torch.from_numpy(taps),
                     'bands': torch.from_numpy(S.band_edges())}
        x = np.random.default_rng(sr).standard_normal(7919)
        err = np.abs(S.resample(x, p, q, taps) - S.resample_upfirdn(x, p, q, taps)).max()
        assert err <= 1e-13 * np.abs(x).max(), (sr, err)
    assert plans[10000]['taps'].tolist() == [1.0] and plans[44100]['taps'].numel() == 8821

    d, stages, margins = {}, {}, {}
    for name in cases:
        ref, deg, sr = case_signals(fx, name)
        st = S.stoi_stages(ref, deg, sr)
        d[name] = st['d']
        margins[name] = threshold_margin(st['energy'])
        assert margins[name] > 1e-6, (name, margins[name])
        if name in STAGE_CASES:
            stages[name] = {k: torch.from_numpy(np.ascontiguousarray(st[k])) for k in
                            ('xr', 'yr', 'energy', 'xs', 'ys', 'X', 'Y', 'rho')}
            stages[name]['mask'] = torch.from_numpy(st['mask'].astype(np.int32))
            stages[name]['M'] = st['M']
            stages[name]['d'] = st['d']
            assert 0 < st['M'] < len(st['mask']) and st['rho'].shape[0] > 0, name
        if name == 'zero_run':
            Y = st['Y']
            allzero = [(i, m) for i in range(S.J) for m in range(S.SEG - 1, Y.shape[1])
                       if not Y[i, m - S.SEG + 1:m + 1].any()]
            assert allzero, 'zero_run has no all-zero processed window'
            fx['zero_run_windows'] = len(allzero)
    assert math.isnan(d['short']) and math.isnan(d['silent'])
    assert all(math.isfinite(v) for k, v in d.items() if k not in ('short', 'silent')), d
    snr_d = [d['snr{}'.format(s).replace('-', 'm')] for s in SNRS]
    assert all(a < b for a, b in zip(snr_d, snr_d[1:])), snr_d
    assert abs(d['scaled'] - 1) < 1e-12, d['scaled']

    # eval CLI: three wav pairs of 0.75 s (the second processed file 0.1 s longer: truncated)
    names, cl, no, cd = [], [], [], []
    for k, (a, snr) in enumerate(((0, 0), (int(1.1 * SR), 10), (int(2.2 * SR), 20))):
        L = int(0.75 * SR)
        cw = clean16[a:a + L]
        extra = int(0.1 * SR) if k == 1 else 0
        nw = to_int16(to_float(clean16[a:a + L + extra]).astype(np.float64) +
                      gain(snr, a, L) * to_float(noise16[a:a + L + extra]))
        Lc = min(len(cw), len(nw))
        cd.append(S.stoi(to_float(cw)[:Lc], to_float(nw)[:Lc], SR))
        names.append('p{:03d}_{:03d}.wav'.format(k + 1, 7 * k + 3))
        cl.append(torch.from_numpy(cw.copy()))
        no.append(torch.from_numpy(nw))
    assert all(math.isfinite(v) for v in cd), cd

    fx.update(plans=plans, d=d, stages=stages, margins=margins,
              cli={'names': names, 'clean': cl, 'noisy': no, 'd': torch.tensor(cd)},
              meta={'recipe': 'scripts/make_golden_stoi.py', 'oracle': 'scripts/stoi_oracle.py',
                    'numpy': np.__version__})
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')
    for k in cases:
        print('  {:9s} d = {:.6f}  margin {:.3g} dB'.format(k, d[k], margins[k]))
    print('  cli', ['{:.4f}'.format(v) for v in cd])


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'stoi.pt'))
