"""Writes tests/golden/reverb.pt: the fixture of the reverberation augmentation (ops.reverb_rows,
augment.RIRBank / Reverb).  Nothing in the reference does this, so the
results are those of the float64 numpy oracle scripts/reverb_oracle.py, asserted here against
scipy.signal.fftconvolve on every case.

    python scripts/make_golden_reverb.py [out.pt]

The file holds recipes and float64 results only: signals and impulse responses are regenerated
from seeds by `case_signal` / `rir_bank` (the sha256 of their bytes is stored).  Of a long row
every `STEP`-th output sample is stored.

The sizes sit on the block and partition boundaries of the kernels for a partition of 128 samples
(ops.REVERB_P): T in {1, 127, 128, 129, 1000, 16384}, taps in {1, 2, 128, 129, 300, 4099} (1, 2, 3
and 33 partitions), the direct path at tap 0, at the last tap and in the middle.  The probe
responses are integers of magnitude 1 .. 8 with the one 8 on the direct path: normalised they are
exact multiples of 1/8, and against a unit impulse every tap shows on its own.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import reverb_oracle as R  # noqa: E402

STEP = 37      # long rows: y[::STEP] is stored

# the bank of the fixture: decaying noise ('decay') or integer probes ('probe'), peak at d
BANK = (
    dict(kind='decay', taps=1, d=0, seed=201),
    dict(kind='decay', taps=2, d=1, seed=202),
    dict(kind='decay', taps=128, d=0, seed=203),
    dict(kind='decay', taps=128, d=127, seed=204),
    dict(kind='decay', taps=129, d=128, seed=205),
    dict(kind='decay', taps=129, d=64, seed=206),
    dict(kind='decay', taps=300, d=150, seed=207),
    dict(kind='decay', taps=300, d=0, seed=208),
    dict(kind='decay', taps=4099, d=0, seed=209),
    dict(kind='decay', taps=4099, d=4098, seed=210),
    dict(kind='decay', taps=4099, d=2049, seed=211),
    dict(kind='decay', taps=100, d=3, seed=212),
    dict(kind='probe', taps=300, d=0, seed=213),
    dict(kind='probe', taps=4099, d=2049, seed=214),
    dict(kind='probe', taps=129, d=128, seed=215),
)

# x: 'gauss' (seeded) or a unit impulse at n0 ('last' = len - 1); prev: the sample before the row
CASES = {
    'T1_L1': dict(T=1, rir=0, seed=1, prev=0.5),
    'T1_L300': dict(T=1, rir=6, seed=2, prev=-0.25),
    'T127_L2': dict(T=127, rir=1, seed=3),
    'T127_L128': dict(T=127, rir=3, seed=4, prev=0.125),
    'T128_L1': dict(T=128, rir=0, seed=5),
    'T128_L128': dict(T=128, rir=2, seed=6, prev=-0.75),
    'T129_L129_len1': dict(T=129, rir=4, seed=7, prev=0.3, length=1),
    'T129_L4099': dict(T=129, rir=10, seed=8, prev=0.2),
    'T1000_L300_len777': dict(T=1000, rir=6, seed=9, prev=-0.4, length=777),
    'T1000_L4099': dict(T=1000, rir=8, seed=10),
    'T1000_L129': dict(T=1000, rir=5, seed=11, prev=0.6, length=129),
    'T16384_L4099_last': dict(T=16384, rir=9, seed=12, prev=0.1),
    'T16384_L129_len16000': dict(T=16384, rir=5, seed=13, length=16000),
    'T16384_L300': dict(T=16384, rir=7, seed=14, prev=-0.2),
    'probe300_n0': dict(T=1000, rir=12, n0=0),
    'probe300_n127': dict(T=1000, rir=12, n0=127),
    'probe300_n128': dict(T=1000, rir=12, n0=128),
    'probe300_last': dict(T=1000, rir=12, n0='last', length=900),
    'probe4099_n0': dict(T=16384, rir=13, n0=0),
    'probe4099_n127': dict(T=16384, rir=13, n0=127),
    'probe4099_n128': dict(T=16384, rir=13, n0=128),
    'probe4099_last': dict(T=16384, rir=13, n0='last'),
    'probe129_n128': dict(T=129, rir=14, n0=128),
    'probe129_n0': dict(T=129, rir=14, n0=0),
}

# one call whose rows use responses of 1, 3 and 33 partitions with different delays, a row whose
# id is outside the bank (returned unchanged, flagged) and rows of different lengths
BATCH = dict(T=1000, seed=50, rirs=[10, 11, 6, len(BANK) + 5, 8, 2], prev=True,
             lengths=[1000, 640, 1, 500, 999, 128])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def raw_rir(rc):
    """The RIR of a bank recipe before the bank's normalisation (float64)."""
    rng = np.random.default_rng(rc['seed'])
    L, d = rc['taps'], rc['d']
    if rc['kind'] == 'probe':
        h = rng.integers(1, 8, size=L).astype(np.float64) * rng.choice([-1.0, 1.0], size=L)
        h[d] = -8.0 if rc['seed'] % 2 else 8.0
        return h
    t = np.arange(L, dtype=np.float64)
    h = rng.standard_normal(L) * np.exp(-np.abs(t - d) / max(L / 6.0, 1.0)) * 0.3
    h[d] = (-1.0 if rc['seed'] % 2 else 1.0) * (1.5 * np.abs(h).max() + 0.1)
    return h


def rir_bank():
    """The fixture's RIRs as float64 arrays, un-normalised (what RIRBank is given)."""
    return [raw_rir(rc) for rc in BANK]


def case_signal(rc):
    """(x float32 [T], length or None, prev float32 or None) of a case recipe."""
    T = rc['T']
    n = rc.get('length', T)
    if 'n0' in rc:
        x = np.zeros(T, np.float32)
        x[n - 1 if rc['n0'] == 'last' else rc['n0']] = 1.0
    else:
        x = (0.3 * np.random.default_rng(rc['seed']).standard_normal(T)).astype(np.float32)
    prev = np.float32(rc['prev']) if 'prev' in rc else None
    return x, rc.get('length'), prev


def batch_signal():
    rng = np.random.default_rng(BATCH['seed'])
    x = (0.3 * rng.standard_normal((len(BATCH['rirs']), BATCH['T']))).astype(np.float32)
    prev = (0.3 * rng.standard_normal(len(BATCH['rirs']))).astype(np.float32)
    return x, prev


def against_fft(x, h, d, length, prev):
    """The oracle's definition through scipy.signal.fftconvolve (float64)."""
    from scipy.signal import fftconvolve
    n = len(x) if length is None else length
    xe = np.concatenate(([0.0 if prev is None else float(prev)], np.asarray(x, np.float64)[:n]))
    full = fftconvolve(xe, np.asarray(h, np.float64))
    y = np.zeros(len(x))
    y[:n] = full[d + 1:d + 1 + n]
    return y, float(full[d])


def stored(y):
    return y if len(y) <= 1000 else y[::STEP]


def main(out):
    import torch
    bank = [R.normalise(h) for h in rir_bank()]
    for rc, (h, d) in zip(BANK, bank):
        assert d == rc['d'] and len(h) == rc['taps'] and h[d] == np.float32(1.0), rc
        if rc['kind'] == 'probe':
            assert np.array_equal(h * 8, np.rint(h * 8)) and np.abs(h).min() >= 0.125, rc
    fx = {'bank': list(BANK), 'cases': CASES, 'batch': BATCH, 'step': STEP,
          'rir_sha': [sha(h) for h, _ in bank], 'sha': {}, 'y': {}, 'prev_out': {}, 'scale': {},
          'fft_err': {}}
    for name, rc in CASES.items():
        x, length, prev = case_signal(rc)
        h, d = bank[rc['rir']]
        y, p = R.reverb(x, h, d, length, prev)
        s = R.scale(x, h, d, length, prev)
        yf, pf = against_fft(x, h, d, length, prev)
        err = max(np.abs(y - yf).max(), abs(p - pf)) / s
        assert err < 1e-13, (name, err)
        if 'n0' in rc:      # the shifted response itself, and the scale is its peak
            assert s == 1.0 and np.array_equal(y * 8, np.rint(y * 8)), name
        fx['sha'][name] = sha(x)
        fx['y'][name] = torch.from_numpy(stored(y).copy())
        fx['prev_out'][name], fx['scale'][name], fx['fft_err'][name] = p, s, float(err)
        print('  {:22s} T {:5d} taps {:4d} d {:4d} scale {:.4f} fftconvolve {:.1e}'.format(
            name, rc['T'], len(h), d, s, err))
    xb, pb = batch_signal()
    fx['sha']['batch'] = sha(xb)
    ys, ps = [], []
    for r, rid in enumerate(BATCH['rirs']):
        if rid >= len(bank):
            ys.append(xb[r].astype(np.float64))
            ps.append(float(pb[r]))
            continue
        h, d = bank[rid]
        y, p = R.reverb(xb[r], h, d, BATCH['lengths'][r], pb[r])
        yf, pf = against_fft(xb[r], h, d, BATCH['lengths'][r], pb[r])
        assert max(np.abs(y - yf).max(), abs(p - pf)) < 1e-13 * R.scale(
            xb[r], h, d, BATCH['lengths'][r], pb[r]), r
        ys.append(y)
        ps.append(p)
    fx['y']['batch'] = torch.from_numpy(np.stack(ys))
    fx['prev_out']['batch'] = ps
    fx['meta'] = {'recipe': 'scripts/make_golden_reverb.py', 'numpy': np.__version__}
    torch.save(fx, out)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else
         os.path.join(ROOT, 'tests', 'golden', 'reverb.pt'))
