"""Writes tests/golden/distort.pt: the fixture of the three signal-level distortions (ops.clip_rows,
ops.chop_rows, ops.fir_rows, augment.Clip / Chop / BandLimit), computed by
the float64 numpy oracle scripts/distort_oracle.py.

    python scripts/make_golden_distort.py [out.pt]

The file holds recipes and results only: signals are regenerated from seeds by `signal` (sha256 of
their bytes is stored).  The chop cases restate their level inputs, the P.56 envelope q and the
threshold c0, with scripts/additive_oracle.py.

Knife-edge condition asserted on every chop case (a condition on the inputs, not a tolerance):
min_t |q[t] - c0| > 1e-9 max q.  The device envelope is within 1e-12 of its peak and c0 within 1e-13
relative of the oracle's, so the set of active samples is the oracle's.  As
in scripts/make_golden_additive.py, every comparison of the level's finalisation and of bin_interp
also clears its bound by more than 1e-6 dB, so that c0 comes out of the same branch.  A candidate
signal that misses a margin is replaced by another seed; the margins stay.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import additive_oracle as A  # noqa: E402
import distort_oracle as D  # noqa: E402
from make_golden_additive import speech_like  # noqa: E402

MARGIN = 1e-9
INTERP_MARGIN_DB = 1e-6
SRATE = 16000
FIR_TILE = 1024

# T = 1, 77, 2048 + 3, 16384; a factor of exactly 1; an all-zero row; len < T; len = 0; |prev| > thr
CLIP_CASES = {
    'one': dict(T=1, seed=21, factor=0.5, prev=0.9),
    'short': dict(T=77, seed=22, factor=0.3, prev=-0.45),
    'odd': dict(T=2051, seed=23, factor=0.1, prev=0.001),
    'full': dict(T=16384, seed=24, factor=0.4, prev=0.5),
    'factor1': dict(T=2051, seed=25, factor=1.0, prev=0.7),
    'zeros': dict(T=77, seed=26, factor=0.2, scale=0.0, prev=0.3),
    'partial': dict(T=2051, seed=27, factor=0.2, length=1500, prev=-0.25),
    'empty': dict(T=77, seed=28, factor=0.2, length=0, prev=0.1),
}

# end to end through augment.Chop: (u, dur) per slot; dur 0 = unused
CHOP_CASES = {
    # first sample, a later slab, the last active sample (u n rounds to n - 1 or is cut to it)
    'spread': dict(T=16384, seed=60, u=[0.0, 0.5, 1.0 - 2.0 ** -53], dur=[800, 1600, 4000]),
    # two overlapping chunks and an unused slot between used ones
    'overlap': dict(T=16384, seed=32, u=[0.30, 0.9, 0.31, 0.6], dur=[3000, 0, 3000, 10]),
    # T no multiple of the slab, len < T, a chunk running past len
    'partial': dict(T=5000, seed=33, length=4100, u=[0.97], dur=[4800]),
    # eight slots
    'eight': dict(T=16384, seed=34, u=[0.05, 0.15, 0.3, 0.45, 0.55, 0.7, 0.85, 0.95],
                  dur=[800, 900, 1000, 1100, 1200, 1300, 1400, 1500]),
    # no level: digital silence, and a level below the P.56 margin
    'zeros': dict(T=5000, seed=35, scale=0.0, u=[0.5], dur=[800]),
    'low': dict(T=16384, seed=36, scale=0.0008, u=[0.5, 0.2], dur=[800, 800]),
}

# one-sided filters: explicit taps, or a low-pass of distort_oracle.lowpass(fc, SRATE, zeros)
FILTERS = (dict(taps=[1.0]),                       # K = 0: the identity
           dict(taps=[0.5, 0.25]),                 # K = 1
           dict(fc=1000.0, zeros=32),              # K = 256
           dict(fc=4000.0, zeros=32),              # K = 64
           dict(fc=125.0, zeros=32))               # K = 2048
FIR_CASES = {
    'identity': dict(T=300, seed=41, filt=0, prev=0.25),
    'k1': dict(T=300, seed=42, filt=1, prev=-0.5),
    'k_over_T': dict(T=77, seed=43, filt=2, prev=0.3),
    'k_over_T_noprev': dict(T=77, seed=43, filt=2),
    'kmax_tile': dict(T=FIR_TILE + 1, seed=44, filt=4, prev=0.2),
    'partial': dict(T=2051, seed=45, filt=3, length=1300, prev=-0.1),
    'empty': dict(T=77, seed=46, filt=3, length=0, prev=0.6),
}
# rows of one batch with different filters, lengths and an id outside the bank
FIR_BATCH = dict(T=2051, seeds=[51, 52, 53, 54, 55], filt=[3, 0, 2, len(FILTERS), 1],
                 lengths=[2051, 2000, 1025, 2051, 7], prev=[0.1, -0.2, 0.3, 0.4, -0.5])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def signal(rc):
    """The float32 signal of a case recipe (speech-like, peak 0.5 times `scale`)."""
    return (speech_like(rc['T'], SRATE, rc['seed']) * np.float32(rc.get('scale', 1.0))).astype(
        np.float32)


def filters():
    """[(K, h[0 .. K])] of FILTERS."""
    out = []
    for f in FILTERS:
        if 'taps' in f:
            h = np.asarray(f['taps'], dtype=np.float64)
            out.append((len(h) - 1, h))
        else:
            out.append(D.lowpass(f['fc'], SRATE, f['zeros']))
    return out


def filter_bank():
    """(bank float64 [nf, Kmax + 1], K int32 [nf]) of FILTERS, as ops.fir_rows takes them."""
    fl = filters()
    bank = np.zeros((len(fl), max(K for K, _ in fl) + 1))
    for f, (K, h) in enumerate(fl):
        bank[f, :K + 1] = h
    return bank, np.asarray([K for K, _ in fl], dtype=np.int32)


def fir_prev(rc):
    """The sample preceding a FIR case's row, as the float32 the device is given (None: absent)."""
    return None if 'prev' not in rc else np.float32(rc['prev'])


def chop_level(x, length=None):
    """(q, c0, margin) of a chop case: the oracle's envelope (zero past the length) and threshold,
    and min |q - c0| / max q over the row's samples (inf without a level)."""
    n = len(x) if length is None else length
    trace = []
    o = A.asl_p56(x[:n], SRATE, trace=trace)
    assert not trace or min(trace) > INTERP_MARGIN_DB, min(trace)
    q = np.zeros(len(x))
    q[:n] = o['q']
    if o['c0'] is None or n == 0:
        return q, None, np.inf
    return q, o['c0'], float(np.abs(o['q'] - o['c0']).min() / o['q'].max())


def chop_case(rc):
    x = signal(rc)
    q, c0, margin = chop_level(x, rc.get('length'))
    return x, q, c0, margin, D.chop(x, q, c0, rc['u'], rc['dur'], rc.get('length'))


def main(out):
    import torch
    fx = {'clip_cases': CLIP_CASES, 'chop_cases': CHOP_CASES, 'filters': list(FILTERS),
          'fir_cases': FIR_CASES, 'fir_batch': FIR_BATCH, 'margin': MARGIN,
          'sha': {}, 'clip': {}, 'chop': {}, 'fir': {}}
    for name, rc in CLIP_CASES.items():
        x = signal(rc)
        o = D.clip(x, rc['factor'], rc.get('length'), rc['prev'])
        fx['sha']['clip_' + name] = sha(x)
        fx['clip'][name] = dict(m=float(o['m']), thr=float(o['thr']), prev=float(o['prev']),
                                nclipped=o['nclipped'], status=o['status'], y_sha=sha(o['y']))
        print('  clip {:9s} m {:.6f} thr {:.6f} nclipped {} status {}'.format(
            name, o['m'], o['thr'], o['nclipped'], o['status']))
    c = fx['clip']
    assert c['factor1']['nclipped'] == 0 and c['factor1']['status'] == 0
    assert c['zeros']['status'] == c['empty']['status'] == D.CLIP_SILENT
    assert 0 < c['partial']['nclipped'] < 1500 and c['full']['nclipped'] > 100
    assert all(abs(CLIP_CASES[k]['prev']) > c[k]['thr'] for k in ('one', 'short', 'full'))
    assert abs(CLIP_CASES['odd']['prev']) < c['odd']['thr']

    for name, rc in CHOP_CASES.items():
        x, q, c0, margin, o = chop_case(rc)
        assert margin > MARGIN, (name, margin)      # pick another seed; never relax
        fx['sha']['chop_' + name] = sha(x)
        fx['chop'][name] = dict(c0=float('nan') if c0 is None else c0, margin=margin,
                                starts=o['starts'].tolist(), nactive=o['nactive'],
                                nzeroed=o['nzeroed'], status=o['status'], y_sha=sha(o['y']))
        print('  chop {:9s} c0 {} n {} starts {} zeroed {} margin {:.2e}'.format(
            name, c0, o['nactive'], o['starts'].tolist(), o['nzeroed'], margin))
    h = fx['chop']
    sp = h['spread']
    assert sp['starts'][0] < 1024 < sp['starts'][1] and sp['status'] == 0
    xs, qs, cs, _, _ = chop_case(CHOP_CASES['spread'])
    assert sp['starts'][2] == np.nonzero(qs >= cs)[0][-1]          # k = n - 1
    ov = h['overlap']
    assert ov['starts'][1] == -1 and abs(ov['starts'][0] - ov['starts'][2]) < 3000
    assert ov['nzeroed'] < 6010
    pa = h['partial']
    assert pa['starts'][0] + 4800 > 4100 and pa['nzeroed'] == 4100 - pa['starts'][0]
    assert len(h['eight']['starts']) == 8 and min(h['eight']['starts']) >= 0
    for k in ('zeros', 'low'):
        assert h[k]['status'] == D.CHOP_NOLEVEL and h[k]['nzeroed'] == 0 and np.isnan(h[k]['c0'])

    fl = filters()
    assert [K for K, _ in fl] == [0, 1, 256, 64, 2048]
    fx['K'] = [K for K, _ in fl]
    fx['filter_sha'] = [sha(hh) for _, hh in fl]
    for name, rc in FIR_CASES.items():
        x = signal(rc)
        K, hh = fl[rc['filt']]
        y, p = D.fir(x, hh, rc.get('length'), fir_prev(rc))
        yc, pc = D.fir_convolve(x, hh, rc.get('length'), fir_prev(rc))
        bound = D.fir_bound(hh, max(np.abs(x).max(), abs(float(fir_prev(rc) or 0.0))))
        dev = max(np.abs(y - yc).max(), abs(p - pc))
        assert dev <= bound, (name, dev, bound)
        fx['sha']['fir_' + name] = sha(x)
        fx['fir'][name] = dict(y=torch.from_numpy(y), prev=float(p), bound=bound, convolve_dev=dev)
        print('  fir  {:15s} K {:4d} |same-order - convolve| {:.2e} bound {:.2e}'.format(
            name, K, dev, bound))
    assert np.array_equal(fx['fir']['identity']['y'].numpy(),
                          signal(FIR_CASES['identity']).astype(np.float64))
    fx['meta'] = {'recipe': 'scripts/make_golden_distort.py', 'numpy': np.__version__}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(ROOT, 'tests', 'golden', 'distort.pt'))
