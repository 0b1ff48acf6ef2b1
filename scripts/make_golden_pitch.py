"""Writes tests/golden/pitch.pt: the fixture of ops.pitch / ops.pitch_stages / ops.f0_eval and
quality.pitch / quality.f0_eval, computed with the numpy oracle scripts/pitch_oracle.py (DESIGN.md
section 19).

    python scripts/make_golden_pitch.py [out.pt]

Everything is synthetic (seeded numpy) and stored as float32, so that no sine of another machine's
libm enters a test:

  signals   glide (a harmonic glide 90 -> 300 Hz at 20 dB SNR, 16384 samples), speech (a gated
            signal: silence, voiced, unvoiced, voiced, silence, voiced), noise (white), speech8
            (the like of speech at 8 kHz, 6000 samples)
  gains     the noise gains that put speech + g noise at 20, 10 and 5 dB SNR
  ragged    the contours of glide[:L] for the lengths where the indexing can go wrong, d' and its
            cancellation scale for the short ones
  tracks    the contours of speech at theta = 0.15, 0.1 and 0.3, of its noisy versions and of
            the noise, and of speech8 at 8 kHz (with d' of its first 1000 samples)
  evals     the four measures of (speech, each of the processed signals)
  meta      what the tolerances of the GPU tests rest on: for each quantity the largest movement
            of the oracle between float64 and numpy.longdouble (d' and ap relative to the
            cancellation scale (E(0) + E(tau)) tau / c(tau), f0 relative, f0_mae and f0_kld
            relative to max(|value|, 1)), and the smallest decision margin of any frame

It asserts that no frame of any contour has a decision margin below 1e-7 (and moves on to the next
seed if one does), and that float64 and longdouble agree on every lag.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pitch_oracle as O  # noqa: E402

SEED = 20261
MARGIN = 1e-7
N = 16384
LENGTHS = (0, 266, 347, 666, 667, 747, 4001, 16384)
CMND_UP_TO = 4001            # d' is stored for the rows of at most this many samples
THETAS = (0.15, 0.1, 0.3)
SNRS = (20, 10, 5)
N8, N8_SHORT = 6000, 1000


def harmonics(f0, srate, nharm=8):
    """sum_h sin(h phase) / h with the instantaneous frequency f0 [n], below srate / 2."""
    phase = 2 * np.pi * np.cumsum(f0) / srate
    x = np.zeros(len(f0))
    for h in range(1, nharm + 1):
        x += np.where(h * f0 < srate / 2, np.sin(h * phase) / h, 0.0)
    return x


def _fade(n, srate):
    k = min(int(0.01 * srate), n // 2)
    w = np.ones(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(k) + 0.5) / k)
    w[:k], w[n - k:] = ramp, ramp[::-1]
    return w


def gated(n, srate, rng):
    """silence, voiced 120 -> 160 Hz, unvoiced, voiced 200 -> 140 Hz, silence, voiced 100 Hz;
    digital zeros in the silences."""
    cut = [int(round(c * n)) for c in (0.0, 0.09, 0.37, 0.49, 0.79, 0.885, 1.0)]
    x = np.zeros(n)
    for (a, b), kind in zip(zip(cut[:-1], cut[1:]),
                            (None, (120, 160), 'noise', (200, 140), None, (100, 100))):
        m = b - a
        if kind is None:
            continue
        if kind == 'noise':
            seg = 0.05 * rng.standard_normal(m)
        else:
            seg = 0.3 * harmonics(np.geomspace(kind[0], kind[1], m), srate)
            seg = seg + 10 ** (-30 / 20) * np.sqrt(np.mean(seg ** 2)) * rng.standard_normal(m)
        x[a:b] = seg * _fade(m, srate)
    return x


def make_signals(seed):
    rng = np.random.default_rng(seed)
    g = 0.3 * harmonics(np.geomspace(90, 300, N), 16000)
    g = g + 10 ** (-20 / 20) * np.sqrt(np.mean(g ** 2)) * rng.standard_normal(N)
    sig = {'glide': g, 'speech': gated(N, 16000, rng), 'noise': 0.1 * rng.standard_normal(N),
           'speech8': gated(N8, 8000, rng)}
    return {k: v.astype(np.float32) for k, v in sig.items()}


def snr_gain(clean, noise, snr_db):
    c, n = clean.astype(np.float64), noise.astype(np.float64)
    return float(np.sqrt(np.sum(c * c) / (np.sum(n * n) * 10.0 ** (snr_db / 10.0))))


def mix(clean, noise, gain):
    """float32(clean + gain noise), the sum in float64."""
    return (clean.astype(np.float64) + gain * noise.astype(np.float64)).astype(np.float32)


def processed(signals, gains):
    """name -> the processed versions of speech."""
    out = {'snr{}'.format(s): mix(signals['speech'], signals['noise'], gains['snr{}'.format(s)])
           for s in SNRS}
    out['noise'] = signals['noise']
    return out


def ap_scale(tr, srate):
    """per frame, the largest cancellation scale over the lag range: what ap moves with"""
    _, tmin, tmax = O.constants(srate)
    s = tr['scale'][:, tmin:tmax + 1]
    return s.max(axis=1) if len(s) else np.zeros(0)


def track_gap(a, b, srate):
    """The movement between two runs of the oracle (float64, longdouble) of one row: d' and ap
    relative to the cancellation scale, f0 relative."""
    assert np.array_equal(a['lag'], b['lag'])
    g = {'cmnd': 0.0, 'ap': 0.0, 'f0': 0.0}
    if len(a['lag']) == 0:
        return g
    sc = np.asarray(b['scale'], np.float64)
    diff = np.abs(np.asarray(a['cmnd'] - b['cmnd'], np.float64))
    assert not diff[sc == 0].any()
    g['cmnd'] = float(np.max(diff[sc > 0] / sc[sc > 0])) if (sc > 0).any() else 0.0
    s = ap_scale(a, srate)
    da = np.abs(np.asarray(a['ap'] - b['ap'], np.float64))
    assert not da[s == 0].any()
    g['ap'] = float(np.max(da[s > 0] / s[s > 0])) if (s > 0).any() else 0.0
    v = a['lag'] > 0
    if v.any():
        g['f0'] = float(np.max(np.abs(np.asarray(a['f0'] - b['f0'], np.float64))[v] / a['f0'][v]))
    return g


def eval_gap(a, b):
    g = {}
    for k in ('f0_mae', 'f0_kld'):
        x, y = float(a[k]), float(b[k])
        assert math.isnan(x) == math.isnan(y)
        g[k] = 0.0 if math.isnan(x) else float(abs(a[k] - b[k])) / max(abs(x), 1.0)
    for k in ('vuv_acc', 'voiced'):
        assert float(a[k]) == float(b[k]) or (math.isnan(float(a[k])) and math.isnan(float(b[k])))
    return g


def pack(tr, srate, with_cmnd):
    import torch
    out = {'f0': torch.from_numpy(tr['f0'].copy()), 'lag': torch.from_numpy(tr['lag'].copy()),
           'ap': torch.from_numpy(tr['ap'].copy()),
           'ap_scale': torch.from_numpy(np.ascontiguousarray(ap_scale(tr, srate)))}
    if with_cmnd:
        out['cmnd'] = torch.from_numpy(tr['cmnd'].copy())
        out['scale'] = torch.from_numpy(tr['scale'].copy())
    return out


def build(seed):
    """The fixture for `seed`, or None where a frame's decision margin is below MARGIN."""
    import torch
    signals = make_signals(seed)
    gains = {'snr{}'.format(s): snr_gain(signals['speech'], signals['noise'], s) for s in SNRS}
    gaps = {'cmnd': 0.0, 'ap': 0.0, 'f0': 0.0, 'f0_mae': 0.0, 'f0_kld': 0.0}
    margins = []

    def run(x, srate, theta, with_cmnd):
        a = O.track(x, srate, theta)
        b = O.track(x, srate, theta, dtype=np.longdouble)
        for k, v in track_gap(a, b, srate).items():
            gaps[k] = max(gaps[k], v)
        margins.append(a['margin'])
        return a, pack(a, srate, with_cmnd)

    ragged = {L: run(signals['glide'][:L], 16000, O.THETA, 0 < L <= CMND_UP_TO)[1]
              for L in LENGTHS}
    tracks, raw = {}, {}
    for theta in THETAS:
        raw[theta], tracks['speech@{}'.format(theta)] = run(signals['speech'], 16000, theta, False)
    deg = processed(signals, gains)
    evals = {}
    for name, x in deg.items():
        d, tracks[name] = run(x, 16000, O.THETA, False)
        c = raw[O.THETA]
        e64 = O.f0_eval(c['f0'], c['lag'], d['f0'], d['lag'])
        eld = O.f0_eval(c['f0'], c['lag'], d['f0'], d['lag'], dtype=np.longdouble)
        for k, v in eval_gap(e64, eld).items():
            gaps[k] = max(gaps[k], v)
        evals[name] = {k: float(v) for k, v in e64.items()}
    tracks['speech8'] = run(signals['speech8'], 8000, O.THETA, False)[1]
    tracks['speech8_short'] = run(signals['speech8'][:N8_SHORT], 8000, O.THETA, True)[1]
    margin = float(min(m.min() for m in margins if len(m)))
    if margin < MARGIN:
        return None
    return {'signals': {k: torch.from_numpy(v) for k, v in signals.items()}, 'gains': gains,
            'lengths': list(LENGTHS), 'thetas': list(THETAS), 'ragged': ragged, 'tracks': tracks,
            'evals': evals,
            'meta': {'recipe': 'scripts/make_golden_pitch.py', 'oracle': 'scripts/pitch_oracle.py',
                     'seed': seed, 'gaps': gaps, 'min_margin': margin, 'margin_floor': MARGIN,
                     'frames': int(sum(len(m) for m in margins)), 'numpy': np.__version__}}


def main(out):
    import torch
    for seed in range(SEED, SEED + 20):
        fx = build(seed)
        if fx is not None:
            break
        print('seed', seed, 'has a frame with a decision margin below', MARGIN)
    else:
        raise SystemExit('no seed without a close decision')
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes; seed', fx['meta']['seed'])
    print('  frames', fx['meta']['frames'], ' smallest margin', fx['meta']['min_margin'])
    print('  gaps', fx['meta']['gaps'])
    for name, e in fx['evals'].items():
        print('  speech vs {:6s}'.format(name), e)
    for name, t in fx['tracks'].items():
        print('  {:14s} frames {:4d} voiced {:4d}'.format(name, len(t['lag']),
                                                        int((t['lag'] > 0).sum())))


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'pitch.pt'))
