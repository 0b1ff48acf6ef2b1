"""Writes tests/golden/wpe.pt: the fixture of ops.wpe_rows / ops.wpe_stages and baselines.wpe,
computed with the numpy oracle scripts/wpe_oracle.py.

    python scripts/make_golden_wpe.py [out.pt]

Everything is synthetic (seeded numpy) and stored, so that no sine of another machine's libm enters
a test:

  signals   int16 (a row is the signal / 32768 in float32, exactly).  The source is speech-like, 2 s
            at 16 kHz: harmonics of a moving F0 shaped by two moving formants, gated at a syllable
            rate, plus a little noise.  'rev06' and 'rev03' are the source through a synthetic
            exponentially decaying response of RT60 0.6 / 0.3 s: a direct path of gain 1 and a tail
            of the same energy, a direct-to-reverberant ratio of 0 dB (rev03: the first second
            only).  'early06' and 'early03' are the source through the first 32 ms of the same
            response: the early-reflection target.  'rev8' is the like at 8 kHz, 4.1 s, RT60 0.6 s.
            float32: 'band4k' (rev06[:8000] without its bins from 4 kHz up)
  cases     name -> {'srate', 'taps', 'delay', 'iterations', 'nframes', 'status', 'gaps' and a
            subsample of the oracle's float64 'y', 'X' and 'g' (`subsample`)}; the rows themselves
            are made by `case_rows` from the signals.  'gaps' is the movement of the oracle between
            float64 and numpy.longdouble on that row: y relative to max |x|, X relative to
            max |Y|, g absolute.  The GPU tests hold the kernels to 100 times these, per case.
  meta      'improvement_db': by how much WPE with the default parameters lowers the energy of the
            residual against the early-reflection target on rev03 and rev06, measured with the
            float64 oracle here; tests/test_wpe.py asserts half of it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wpe_oracle as O  # noqa: E402

SEED = 20263
N = 32000
N8 = 32577                   # 513 frames at 8 kHz: one above the kernel's frame tile of 512
TILE = 512
LENGTHS = (1, 127, 128, 129, 1280, 1281, 8000, 32000)
EARLY_MS = 32
DEFAULTS = {'taps': 10, 'delay': 3, 'iterations': 3}
Y_STRIDE, XB_STRIDE, XT_STRIDE, G_STRIDE = 61, 32, 13, 32


def speechlike(n, srate, rng):
    """A source whose pitch and formants move: harmonics of F0(t) weighted by two resonances whose
    centres glide, gated at about four syllables a second, plus noise 40 dB down."""
    t = np.arange(n) / float(srate)
    f0 = 120.0 + 40.0 * np.sin(2 * np.pi * 0.7 * t) + 25.0 * np.sin(2 * np.pi * 2.3 * t + 1.0)
    phase = 2 * np.pi * np.cumsum(f0) / srate
    f1 = 500.0 + 250.0 * np.sin(2 * np.pi * 1.1 * t)
    f2 = 1500.0 + 600.0 * np.sin(2 * np.pi * 0.9 * t + 2.0)
    sig = np.zeros(n)
    for h in range(1, 40):
        fh = h * f0
        if fh.max() >= 0.45 * srate:
            break
        w = 1.0 / (1.0 + ((fh - f1) / 120.0) ** 2) + 0.5 / (1.0 + ((fh - f2) / 200.0) ** 2) + 0.02
        sig += w * np.sin(h * phase + 0.7 * h * h)
    gate = np.clip(1.5 * np.sin(2 * np.pi * 2.0 * t + 0.3) ** 2 - 0.25, 0.0, 1.0)
    sig = sig * gate
    sig = sig / np.abs(sig).max()
    return 0.25 * (sig + 0.01 * rng.standard_normal(n))


def response(rt60, srate, rng):
    """h[0] = 1 and a Gaussian tail with a 60 dB decay over rt60, scaled to the direct path's
    energy."""
    n = int(round(1.2 * rt60 * srate))
    t = np.arange(n) / float(srate)
    h = rng.standard_normal(n) * 10.0 ** (-3.0 * t / rt60)
    h[0] = 0.0
    h = h / np.sqrt(np.sum(h * h))
    h[0] = 1.0
    return h


def make_signals(seed):
    rng = np.random.RandomState(seed)
    dry = speechlike(N, 16000, rng)
    sig = {}
    for name, rt, keep in (('03', 0.3, N // 2), ('06', 0.6, N)):
        h = response(rt, 16000, rng)
        sig['rev' + name] = 0.5 * np.convolve(dry, h)[:keep]
        sig['early' + name] = 0.5 * np.convolve(dry, h[:EARLY_MS * 16])[:keep]
    dry8 = speechlike(N8, 8000, rng)
    sig['rev8'] = 0.5 * np.convolve(dry8, response(0.6, 8000, rng))[:N8]
    out = {k: np.clip(np.rint(v * 32768.0), -32768, 32767).astype(np.int16) for k, v in sig.items()}
    spec = np.fft.rfft(row(out['rev06'])[:8000].astype(np.float64))
    spec[2000:] = 0                              # bin k of 8000 samples is 2 k Hz
    out['band4k'] = np.fft.irfft(spec, 8000).astype(np.float32)
    return out


def row(sig):
    """The float32 row of a stored signal."""
    sig = np.asarray(sig)
    return sig.astype(np.float32) / np.float32(32768) if sig.dtype == np.int16 else sig


def tile_lengths(srate=8000):
    """Rows of one frame below, at and above the kernel's frame tile."""
    H = O.constants(srate)[1]
    return tuple((nf - 3 - 1) * H + off for nf, off in ((TILE - 1, H), (TILE, H), (TILE + 1, 1)))


def case_rows(signals):
    """name -> (row float32, srate, parameters): every case of the GPU test."""
    x = row(signals['rev06'])
    x8 = row(signals['rev8'])
    rows = {'L{}'.format(L): (x[:L].copy(), 16000, DEFAULTS) for L in LENGTHS}
    rows['rate8'] = (x8[:8000].copy(), 8000, DEFAULTS)
    rows['zero'] = (np.zeros(8000, np.float32), 16000, DEFAULTS)
    s = x[:8000].copy()
    s[:3000] = 0
    rows['silent_start'] = (s, 16000, DEFAULTS)
    rows['scaled'] = (x[:8000] * np.float32(2.0 ** -10), 16000, DEFAULTS)
    rows['band4k'] = (np.asarray(signals['band4k'], np.float32).copy(), 16000, DEFAULTS)
    for key, vals in (('taps', (1, 32)), ('delay', (1, 8)), ('iterations', (0, 1))):
        for v in vals:
            rows['{}{}'.format(key, v)] = (x[:8000].copy(), 16000, dict(DEFAULTS, **{key: v}))
    for L in tile_lengths():
        rows['tile8_L{}'.format(L)] = (x8[:L].copy(), 8000, DEFAULTS)
    return rows


def subsample(r):
    """What the fixture keeps of a run of the oracle."""
    y = np.asarray(r['y'], np.float64)
    return {'y': y.copy() if len(y) <= 1281 else y[::Y_STRIDE].copy(),
            'X': np.asarray(r['X'], np.complex128)[::XB_STRIDE, ::XT_STRIDE].copy(),
            'g': np.asarray(r['g'], np.complex128)[::G_STRIDE].copy()}


def errors(a, b, x):
    """{'y', 'X', 'g'}: the distance of run a from run b on the row x, as the gaps are defined."""
    f = lambda v: float(np.max(np.abs(v))) if v.size else 0.0   # noqa: E731
    peak, ypeak = f(np.asarray(x, np.float64)), f(np.asarray(b['Y']))
    dy, dX, dg = (f(np.asarray(a[k] - b[k])) for k in ('y', 'X', 'g'))
    assert (peak > 0 or dy == 0) and (ypeak > 0 or dX == 0)
    return {'y': dy / peak if peak > 0 else 0.0, 'X': dX / ypeak if ypeak > 0 else 0.0, 'g': dg}


def residual_db(x, early):
    e = np.asarray(x, np.float64) - np.asarray(early, np.float64)
    return 10.0 * np.log10(np.sum(e * e))


def improvement_db(signals, name, **kw):
    """By how many dB WPE lowers the energy of (signal - early target) on 'rev' + name."""
    x, early = row(signals['rev' + name]), row(signals['early' + name])
    y = O.wpe(x, 16000, **dict(DEFAULTS, **kw))['y']
    return residual_db(x, early) - residual_db(y, early)


def build(seed):
    import torch
    signals = make_signals(seed)
    cases = {}
    for name, (x, srate, kw) in case_rows(signals).items():
        a = O.wpe(x, srate, **kw)
        b = O.wpe(x, srate, dtype=np.longdouble, **kw)
        assert a['nframes'] == b['nframes'] and a['status'] == b['status'] == 0, name
        c = dict(kw, srate=srate, nframes=a['nframes'], status=a['status'], gaps=errors(a, b, x))
        c.update({k: torch.from_numpy(v) for k, v in subsample(a).items()})
        cases[name] = c
    imp = {name: float(improvement_db(signals, name)) for name in ('03', '06')}
    return {'signals': {k: torch.from_numpy(v) for k, v in signals.items()}, 'cases': cases,
            'lengths': list(LENGTHS),
            'meta': {'recipe': 'scripts/make_golden_wpe.py', 'oracle': 'scripts/wpe_oracle.py',
                     'seed': seed, 'improvement_db': imp, 'early_ms': EARLY_MS,
                     'tile': TILE, 'numpy': np.__version__}}


def main(out):
    import torch
    fx = build(SEED)
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes; seed', fx['meta']['seed'])
    print('  improvement against the early target, dB:', fx['meta']['improvement_db'])
    for name, c in fx['cases'].items():
        print('  {:14s} nf {:4d}'.format(name, c['nframes']),
              {k: '{:.2g}'.format(v) for k, v in c['gaps'].items()})


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'wpe.pt'))
