"""Writes tests/golden/additive.pt: the fixture of the additive-noise mixer (ops.asl_p56,
ops.additive_mix, augment.Additive), computed by the REAL reference's
`Additive` (segan/utils.py:43-297 of the reference checkout, imported through
oracle/ref_harness.py).

    python scripts/make_golden_additive.py [out.pt]

The reference object is built with `Additive.__new__` (its constructor needs librosa and a
directory); `np.asscalar` is shimmed; `addnoise_asl`, `asl_P56` and `bin_interp` are wrapped to
record what they were given and returned, and the locals of `asl_P56` (the activity counts `a` and
the envelope `q`, which it does not return) are read at its return through `sys.setprofile`.

Every case is run twice with the same draws: on float64 copies of the float32 signal and noises
(the TRUTH: all float64) and on the float32 arrays as shipped (the LITERAL run, whose `np.dot`
accumulates sq and Pn in float32).  The file holds recipes and results only: signals and noises are
regenerated from seeds by `case_signal` / `noise_bank` (sha256 of their bytes is stored), and the
float64 mix is restated exactly by `truth_mix` from the stored sf and n (elementwise IEEE
operations; the recipe asserts bit equality with what the reference computed).

Knife-edge conditions asserted on every case (conditions on the inputs, not tolerances):
min |q[k] - c_j| / c_j > 1e-9, and every comparison of the finalisation and of bin_interp clears
its bound by more than 1e-6 dB.
"""
import hashlib
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import additive_oracle as A  # noqa: E402

NOISES = ({'seed': 101, 'len': 70000, 'gain': 0.1, 'pole': 0.0},
          {'seed': 102, 'len': 90000, 'gain': 0.02, 'pole': 0.9})
STAGE_CASES = ('ord16k', 'short')      # q stored

CASES = {
    'ord16k': dict(srate=16000, T=16384, seed=1, scale=1.0, draw=11),
    'ord40k': dict(srate=16000, T=40000, seed=3, scale=1.0, draw=12),
    'quiet': dict(srate=16000, T=16384, seed=5, scale=0.01, draw=13),
    'low': dict(srate=16000, T=16384, seed=6, scale=0.0008, draw=14),
    'zeros': dict(srate=16000, T=16384, seed=7, scale=0.0, draw=15),
    'zero_run': dict(srate=16000, T=56000, seed=8, scale=1.0, zero=(16000, 51200), draw=16),
    'extreme': dict(srate=16000, T=16384, seed=2, scale=0.3, draw=17),
    'clip': dict(srate=16000, T=16384, seed=4, scale=1.9, snr_levels=[0], draw=18),
    'short': dict(srate=16000, T=77, seed=9, scale=1.0, draw=19),
    'sr8k': dict(srate=8000, T=16000, seed=10, scale=1.0, draw=20),
}


def speech_like(n, srate, seed):
    """AR resonance at 700 Hz driven by white noise, times a slow syllable envelope; peak 0.5."""
    from scipy.signal import lfilter
    rng = np.random.default_rng(seed)
    w = 2 * np.pi * 700.0 / srate
    x = lfilter([1.0], [1.0, -2 * 0.95 * np.cos(w), 0.95 * 0.95], rng.standard_normal(n))
    t = np.arange(n) / srate
    env = 0.15 + 0.85 * np.abs(np.sin(2 * np.pi * 2.7 * t + rng.uniform(0, np.pi))) ** 1.5
    x = x * env
    return (0.5 * x / np.abs(x).max()).astype(np.float32)


def case_signal(rc):
    """The float32 signal of a case recipe."""
    x = (speech_like(rc['T'], rc['srate'], rc['seed']) * np.float32(rc['scale'])).astype(np.float32)
    if 'zero' in rc:
        x[rc['zero'][0]:rc['zero'][1]] = 0
    return x


def noise_bank():
    """The float32 noises of the fixture (white, and a one-pole coloured one)."""
    from scipy.signal import lfilter
    out = []
    for rc in NOISES:
        w = np.random.default_rng(rc['seed']).standard_normal(rc['len'])
        if rc['pole']:
            w = lfilter([1.0], [1.0, -rc['pole']], w)
        out.append((rc['gain'] * w).astype(np.float32))
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def truth_mix(clean32, seg32, sf, n):
    """float64 clean + segment * sf followed by n successive divisions by 1.1, 1.2, ...: the
    reference's arithmetic on float64 copies, elementwise."""
    v = clean32.astype(np.float64) + seg32.astype(np.float64) * np.float64(sf)
    small = 0.1
    for _ in range(n):
        v = v / (1. + small)
        small = small + 0.1
    return v


def run_reference(U, wav, noises, snr_levels, srate, seed):
    """One `Additive.__call__` of the real reference with everything it computed recorded."""
    add = U.Additive.__new__(U.Additive)
    add.noises = [{'file': 'noise{}'.format(i), 'data': d} for i, d in enumerate(noises)]
    add.snr_levels = snr_levels
    add.do_IRS = False
    add.eps = 1e-22
    rec = {'interp': []}
    code = U.Additive.asl_P56.__code__

    def prof(frame, event, arg):
        if event == 'return' and frame.f_code is code:
            loc = frame.f_locals
            rec['counts'] = np.asarray(loc['a']).astype(np.int64)
            rec['q'] = np.asarray(loc['q']).copy()
            rec['sq'] = loc['sq']
            rec['level'] = arg

    orig_add, orig_interp = add.addnoise_asl, add.bin_interp

    def addnoise(clean, noise, srate_, nbits, snr, do_IRS=False):
        noisy, bounds = orig_add(clean, noise, srate_, nbits, snr, do_IRS=do_IRS)
        rec.update(noisy_pre=np.asarray(noisy).copy(), bounds=bounds, snr=int(np.asarray(snr)[0]),
                   noise_idx=[i for i, d in enumerate(noises) if d is noise][0])
        return noisy, bounds

    def interp(*a):
        rec['interp'].append([float(v) for v in a])
        return orig_interp(*a)

    add.addnoise_asl, add.bin_interp = addnoise, interp
    np.random.seed(seed)
    sys.setprofile(prof)
    try:
        out = add(wav, srate=srate, nbits=16)
    finally:
        sys.setprofile(None)
    rec['out'] = out.numpy()
    return rec


def main(out):
    import torch
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import ref_harness
    ref_harness.import_reference()
    import segan.utils as U
    if not hasattr(np, 'asscalar'):
        np.asscalar = lambda a: a.item()
    np.seterr(all='ignore')

    noises = noise_bank()
    noises64 = [d.astype(np.float64) for d in noises]
    fx = {'cases': CASES, 'noises': list(NOISES), 'noise_sha': [sha(d) for d in noises],
          'truth': {}, 'literal': {}, 'q': {}, 'sha': {}, 'margins': {}}
    for name, rc in CASES.items():
        x = case_signal(rc)
        levels = rc.get('snr_levels', [0, 5, 10])
        tr = run_reference(U, x.astype(np.float64), noises64, levels, rc['srate'], rc['draw'])
        li = run_reference(U, x, noises, levels, rc['srate'], rc['draw'])
        assert tr['bounds'] == li['bounds'] and tr['snr'] == li['snr'], name
        assert tr['noise_idx'] == li['noise_idx'] and (tr['counts'] == li['counts']).all(), name
        s0, s1 = tr['bounds']
        seg = noises[tr['noise_idx']][s0:s1]
        assert s1 - s0 == rc['T'] and len(seg) == rc['T'], name

        # knife edges
        qm = A.threshold_margin(tr['q'])
        assert qm > 1e-9, (name, qm)
        trace = []
        fin = A.finalise(tr['sq'], tr['counts'], rc['T'], 16, trace)
        im = min(trace) if trace else math.inf
        assert im > 1e-6, (name, im)

        def level(rec):
            asl_ms, asl, c0 = rec['level']
            return dict(sq=float(rec['sq']), asl_ms=float(asl_ms), asl=float(asl),
                        c0=float('nan') if c0 is None else float(c0))

        t, l = level(tr), level(li)
        # our finalisation, restated, gives the reference's values exactly
        assert (float(fin[0]), float(fin[1])) == (t['asl_ms'], t['asl']), (name, fin, t)
        assert (fin[2] is None) == math.isnan(t['c0']) and fin[3] == 0, name
        assert (A.activity_counts(tr['q'], rc['srate']) == tr['counts']).all(), name

        def mixinfo(rec, lvl, segx):
            Pn = float(np.dot(segx.T, segx) / rc['T'])
            sf = float(np.sqrt(lvl['asl_ms'] / Pn / (10 ** (np.array([rec['snr']]) / 10)))[0])
            n = A.clip_divisions(rec['noisy_pre'].max(), rec['noisy_pre'].min())
            return dict(Pn=Pn, sf=sf, n=n)

        t.update(mixinfo(tr, t, seg.astype(np.float64)))
        l.update(mixinfo(li, l, seg))
        t64 = truth_mix(x, seg, t['sf'], t['n'])
        pre = truth_mix(x, seg, t['sf'], 0)
        assert np.array_equal(pre, tr['noisy_pre']), name          # bit for bit
        assert np.array_equal(t64.astype(np.float32), tr['out']), name
        assert np.array_equal(truth_mix(x, seg, l['sf'], l['n']).astype(np.float32), li['out']), name
        t.update(counts=torch.from_numpy(tr['counts']), noise_idx=tr['noise_idx'], snr=tr['snr'],
                 start=int(s0), shortcut=False, interp_calls=len(tr['interp']))
        if tr['interp']:
            up, lw, upt, lwt, M, tol = tr['interp'][0]
            t['shortcut'] = bool(abs(up - upt - M) < tol or abs(lw - lwt - M) < tol)
        l['err'] = float(np.abs(li['out'].astype(np.float64) - t64).max())
        t['err32'] = float(np.abs(tr['out'].astype(np.float64) - t64).max())
        fx['truth'][name], fx['literal'][name] = t, l
        fx['sha'][name] = {'signal': sha(x), 'noisy32': sha(tr['out'])}
        fx['margins'][name] = {'q': qm, 'interp_db': im}
        if name in STAGE_CASES:
            fx['q'][name] = torch.from_numpy(tr['q'])
        if name == 'short':
            fx['short_noisy32'] = torch.from_numpy(tr['out'].copy())
        print('  {:9s} asl_ms {:.6e} asl {:.4f} c0 {:.6e} a0 {} n {} snr {} start {} noise {} '
              'margins q {:.2e} interp {:.2e} shortcut {}'.format(
                  name, t['asl_ms'], t['asl'], t['c0'], int(tr['counts'][0]), t['n'], t['snr'],
                  s0, t['noise_idx'], qm, im, t['shortcut']))

    T = fx['truth']
    assert T['zeros']['counts'][0] == 0 and math.isnan(T['zeros']['c0'])
    assert T['low']['counts'][0] > 0 and math.isnan(T['low']['c0']) and T['low']['asl_ms'] == 0
    assert T['extreme']['shortcut'] and T['extreme']['c0'] == 2.0 ** -8
    assert T['clip']['n'] >= 1
    assert all(T[k]['n'] == 0 for k in CASES if k != 'clip')
    assert not T['ord16k']['shortcut'] and T['ord16k']['interp_calls'] == 1
    # hangover: the 2.2 s zero run outlasts the envelope's decay and the 0.2 s hangover, so the
    # lowest count covers the 20800 signal samples plus that tail and stops well short of T
    assert 20800 + 3200 < T['zero_run']['counts'][0] < CASES['zero_run']['T'] - 25000
    fx['meta'] = {'recipe': 'scripts/make_golden_additive.py', 'numpy': np.__version__}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(ROOT, 'tests', 'golden', 'additive.pt'))
