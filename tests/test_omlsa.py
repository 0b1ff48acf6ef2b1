"""Host side of the OM-LSA enhancer with IMCRA noise tracking: the numpy
oracle scripts/omlsa_oracle.py at its edges, the fixture tests/golden/omlsa.pt against its recipe,
what the enhancer is for (noise whose level changes, where the VAD-gated estimate of the Wiener /
log-MMSE baselines stops updating), the header, the binding, the CLI flags and every refusal that
needs no GPU.

The device parity is tests/test_gpu_omlsa.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import denoise_oracle as D  # noqa: E402
import make_golden_omlsa as GO  # noqa: E402
import omlsa_oracle as O  # noqa: E402

SHORT = ('L1919', 'L1920', 'L2079', 'L2080')
CASES = SHORT + ('L8000', 'L32000', 'rate8', 'zero', 'silent_start', 'scaled') + GO.LONG


@pytest.fixture(scope='module')
def ofx():
    return load_golden('omlsa.pt')


@pytest.fixture(scope='module')
def rebuilt(ofx):
    """the recipe run once here, the three oracles on the four long rows included"""
    return GO.build(ofx['meta']['seed'])


def test_sm3_is_the_literal_three_taps_with_the_mirror():
    rng = np.random.default_rng(1)
    for F in (320, 160, 2):
        a = rng.standard_normal(F + 1) * 10.0 ** rng.uniform(-3, 3, F + 1)
        want = np.empty(F + 1)
        for k in range(F + 1):
            lo = a[1] if k == 0 else a[k - 1]
            hi = a[F - 1] if k == F else a[k + 1]
            want[k] = (0.25 * lo + 0.5 * a[k]) + 0.25 * hi
        assert np.array_equal(O.sm3(a), want)
    assert O.sm3(np.ones(5, np.longdouble), np.longdouble).dtype == np.longdouble
    assert np.array_equal(O.sm3(np.ones(321)), np.ones(321))


def test_constants_are_the_issues():
    assert (O.ALPHA_S, O.ALPHA_D, O.ALPHA, O.BETA, O.B_MIN) == (0.9, 0.85, 0.92, 1.47, 1.66)
    assert (O.GAMMA0, O.GAMMA1, O.ZETA0, O.U, O.V) == (4.6, 3.0, 1.67, 8, 15)
    assert abs(O.LN_GMIN - (-1.25) * np.log(10.0)) < 1e-15
    assert abs(np.exp(O.LN_GMIN) - 10 ** -1.25) < 1e-16
    assert (O.XI_MIN, O.GAMMA_MAX, O.LAMBDA_MIN, O.E1_MIN) == (10.0 ** -2.5, 40.0, 2.0 ** -100,
                                                               2.0 ** -40)
    # 199 frames: slot 0 is overwritten a second time at t + 1 = 135
    slots = [((t + 1) // O.V - 1) % O.U for t in range(199) if (t + 1) % O.V == 0]
    assert slots == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4] and 135 // O.V - 1 == O.U


def test_the_minimum_window_is_the_literal_one():
    """_Minimum against the definition written out per frame: the minimum over the current block
    and the U slots, each slot the minimum of one block of V frames."""
    rng = np.random.default_rng(2)
    f = rng.uniform(0.5, 2.0, (200, 3))
    m = O._Minimum()
    s = None
    hist, mact, smin = None, None, None
    for t in range(200):
        got = m.smooth(f[t], 0.9, 1.0 - 0.9)
        if t == 0:
            s = f[0]
            hist, mact, smin = [s] * O.U, s, s
        else:
            s = 0.9 * s + (1.0 - 0.9) * f[t]
            mact, smin = np.minimum(mact, s), np.minimum(smin, s)
        assert np.array_equal(got, s) and np.array_equal(m.min, smin)
        m.roll(t)
        if (t + 1) % O.V == 0:
            hist[((t + 1) // O.V - 1) % O.U] = mact
            smin, mact = np.min(hist, axis=0), s
        assert np.array_equal(m.min, smin) and np.array_equal(m.mact, mact)
    # after U V frames the first frames have left the window: the minimum can rise again
    up = O._Minimum()
    for t in range(2 * O.U * O.V):
        up.smooth(np.array([1.0 if t < 5 else 10.0]), 0.9, 1.0 - 0.9)
        up.roll(t)
    assert up.min[0] > 9.0


def test_short_zero_and_silent_rows(ofx):
    x = ofx['signals']['noisy'].numpy()
    r = O.omlsa(x[:1919])
    assert r['nframes'] == 0 and len(r['presence']) == len(r['rough']) == len(r['noise']) == 0
    assert r['y'].dtype == np.float64 and np.array_equal(r['y'], x[:1919].astype(np.float64))
    assert r['margin'] == np.inf
    assert [O.omlsa(x[:L])['nframes'] for L in (1920, 2079, 2080)] == [11, 11, 12]
    r = O.omlsa(x[:2079])
    assert r['y'][1920:].tolist() == [0.0] * 159 and r['y'][1800:1920].any()
    z = O.omlsa(np.zeros(8000, np.float32))
    assert z['nframes'] == 49 and not z['y'].any() and not z['rough'].any()
    assert np.isfinite(z['presence']).all() and z['margin'] == np.inf     # exact zeros only
    assert np.array_equal(z['noise'], np.full(321, 2.0 ** -100))
    s, _ = GO.case_rows({k: v.numpy() for k, v in ofx['signals'].items()},
                        ofx['gains'])['silent_start']
    assert not s[:3000].any() and s[3000:].any()
    r = O.omlsa(s)
    assert np.isfinite(r['y']).all() and np.isfinite(r['presence']).all()
    assert np.isfinite(r['noise']).all() and not r['y'][:2720].any()
    assert np.abs(r['y'][3200:]).max() > 0.01
    # Smin is an exact zero for the whole row: no bin can be called noise
    assert not r['rough'].any()
    with pytest.raises(ValueError):
        O.omlsa(x, 44100)


def test_rate8_and_the_longdouble_path(ofx):
    x8 = ofx['signals']['noisy8'].numpy()
    a = O.omlsa(x8, 8000)
    assert a['nframes'] == 99 and a['noise'].shape == (161,) and a['rough'].max() <= 161
    b = O.omlsa(x8[:2000], 8000, dtype=np.longdouble)
    assert b['y'].dtype == b['presence'].dtype == b['noise'].dtype == np.longdouble
    c = O.omlsa(x8[:2000], 8000)
    assert np.array_equal(b['rough'], c['rough'])
    assert np.abs((b['y'] - c['y']).astype(np.float64)).max() < 1e-13
    assert ((a['presence'] >= 0) & (a['presence'] <= 1)).all()


def test_fixture_is_what_its_recipe_and_the_oracle_give(ofx, rebuilt):
    """The matrix products go through the BLAS of the machine, whose summation order is its own:
    y, presence and noise are held to the fixture's own float64-to-longdouble movement times 100,
    the frame counts and the rough counts exactly."""
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'omlsa.pt'))
    assert size < 1024 * 1024, size
    assert rebuilt is not None
    assert set(rebuilt['signals']) == set(ofx['signals']) == {'noisy', 'noisy8', 'clean4', 'noise4'}
    for k, v in ofx['signals'].items():
        assert v.dtype == torch.float32 and torch.equal(v, rebuilt['signals'][k]), k
    assert rebuilt['gains'] == ofx['gains'] and rebuilt['lengths'] == ofx['lengths']
    assert tuple(ofx['cases']) == CASES == tuple(rebuilt['cases'])
    meta = ofx['meta']
    assert meta['margin_floor'] == 1e-9 and meta['min_margin'] >= 1e-9
    assert meta['min_margin'] == min(c['margin'] for c in ofx['cases'].values())
    tol = {k: 100 * v for k, v in meta['gaps'].items()}
    assert set(tol) == {'y', 'presence', 'noise'}
    for k, g in meta['gaps'].items():
        # the rounding that the margin has to cover: orders of magnitude below it
        assert 0 < g and 100 * g <= 1e-10 and 100 * g * 1e3 < meta['min_margin'], (k, g)
    rows = GO.case_rows({k: v.numpy() for k, v in ofx['signals'].items()}, ofx['gains'])
    frames = {}
    for name in CASES:
        want, got = ofx['cases'][name], rebuilt['cases'][name]
        x, srate = rows[name]
        nf = frames[name] = want['nframes']
        assert nf == got['nframes'] == O.n_frames(len(x), srate)
        assert want['rough'].dtype == torch.int64 and torch.equal(want['rough'], got['rough'])
        assert len(want['presence']) == len(want['rough']) == nf
        assert ('y' in want) == (name in SHORT)
        if nf == 0:
            assert len(want['noise']) == 0
            continue
        assert len(want['noise']) == srate // 50 + 1
        assert abs(got['margin'] - want['margin']) <= 1e-6 * want['margin'] or (
            got['margin'] == want['margin'] == np.inf)
        dp = (want['presence'] - got['presence']).abs().max().item()
        dn = ((want['noise'] - got['noise']).abs().max() / want['noise'].max()).item()
        assert dp <= tol['presence'] and dn <= tol['noise'], (name, dp, dn)
        if 'y' in want:
            dy = (want['y'] - got['y']).abs().max().item() / float(np.abs(x).max())
            assert dy <= tol['y'], (name, dy)
    assert [frames[n] for n in CASES] == [0, 11, 11, 12, 49, 199, 99, 49, 49, 49] + [399] * 4
    assert np.array_equal(ofx['cases']['L1919']['y'].numpy(), rows['L1919'][0].astype(np.float64))
    # a power of two changes no decision
    assert torch.equal(ofx['cases']['scaled']['rough'], ofx['cases']['L8000']['rough'])
    # the long rows: 5 dB over the voiced samples after 2.5 s, the level changes as described
    sig = {k: v.numpy().astype(np.float64) for k, v in ofx['signals'].items()}
    _, active = GO.gated6()
    late = GO.late_mask(active)
    assert active[:16000].any() and late.sum() > 10000 and not late[:40000].any()
    for kind in GO.LONG:
        nz = rows[kind][0].astype(np.float64) - sig['clean4']
        assert abs(GO.late_snr(sig['clean4'], rows[kind][0], active) - 5.0) < 0.01
        early = 10 * np.log10(np.mean(nz[:16000] ** 2) / np.mean(nz[48000:] ** 2))
        want_db = {'flat': 0.0, 'step_up': -10.0, 'step_down': 10.0}.get(kind)
        if want_db is None:       # the ramp: 10 dB from its first samples to its last
            first = 10 * np.log10(np.mean(nz[:800] ** 2) / np.mean(nz[48000:] ** 2))
            assert -10.5 < first < -9.0 and -8.5 < early < -6.0, (first, early)
        else:
            assert abs(early - want_db) < 0.3, (kind, early)
    for kind, v in meta['late_snr'].items():
        for k, s in v.items():
            assert abs(s - rebuilt['meta']['late_snr'][kind][k]) < 1e-6, (kind, k)


def test_omlsa_follows_a_noise_level_that_changes(ofx, rebuilt):
    """What the enhancer is for.  On the rows whose noise steps up, ramps up or steps down, the
    oracle's SNR over the voiced samples after 2.5 s is strictly above both existing rules'; and
    on step_up the existing oracle's noise estimate takes no frame in after the step at 1.0 s."""
    snr = rebuilt['meta']['late_snr']
    for kind in GO.LONG:
        s = snr[kind]
        print('{:9s} noisy {:.2f} dB: wiener {:.2f}, logmmse {:.2f}, omlsa {:.2f}'.format(
            kind, s['noisy'], s['wiener'], s['logmmse'], s['omlsa']))
        assert abs(s['noisy'] - 5.0) < 0.01
    for kind in ('step_up', 'ramp', 'step_down'):
        s = snr[kind]
        assert s['omlsa'] > s['wiener'] and s['omlsa'] > s['logmmse'], (kind, s)
    sig = {k: v.numpy() for k, v in ofx['signals'].items()}
    x = GO.long_rows(sig, ofx['gains'])['step_up']
    for rule in D.RULES:
        upd = D.denoise(x, 16000, rule)['update']
        first_after = 16000 // 160          # the first frame that starts at 1.0 s
        print('{}: update fires {} times before 1.0 s, {} times after'.format(
            rule, int(upd[:first_after].sum()), int(upd[first_after:].sum())))
        assert upd[:first_after].sum() >= 10 and not upd[first_after:].any()


def test_binding_header_makefile_and_integration_pins():
    from segan_pytorch_amd import _lib, ops
    assert len(_lib.SIGNATURES) == 119 and _lib.ABI_VERSION == 17
    assert list(_lib.EXT_SIGNATURES) == ['segan_wpe_dims', 'segan_wpe']
    assert list(_lib.PYIN_SIGNATURES) == ['segan_pyin_tables', 'segan_pyin_dims', 'segan_pyin']
    assert list(_lib.OMLSA_SIGNATURES) == ['segan_omlsa_dims', 'segan_omlsa']
    assert [len(_lib.OMLSA_SIGNATURES[n][1]) for n in _lib.OMLSA_SIGNATURES] == [4, 14]
    assert dict(_lib.OMLSA_DEFINES) == {'SEGAN_OMLSA_U': 8, 'SEGAN_OMLSA_V': 15}
    assert (ops.OMLSA_U, ops.OMLSA_V) == (O.U, O.V)
    assert not set(_lib.OMLSA_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) |
                                             set(_lib.PYIN_SIGNATURES))
    with pytest.raises(RuntimeError, match='not found'):
        _lib._read_header_file(_lib.OMLSA_HEADER_PATH + '.missing')
    with open(_lib.OMLSA_HEADER_PATH) as f:
        text = f.read()
    assert 'SEGAN_ABI_VERSION stays 17' in text and 'purely additive' in text
    assert 'SEGAN_ABI_VERSION' not in _lib.OMLSA_DEFINES
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    assert lib.segan_omlsa.argtypes == _lib.OMLSA_SIGNATURES['segan_omlsa'][1]
    assert lib.segan_omlsa_dims.restype is ctypes.c_int and lib.segan_omlsa.restype is ctypes.c_int
    with open(os.path.join(ROOT, 'Makefile')) as f:
        mk = f.read()
    assert '$(CSRC)/segan_omlsa.hip' in mk.split('SRCS :=')[1].split('\n')[0]
    rule = [l for l in mk.split('\n') if l.startswith('$(CSRC)/%.o:')][0]
    assert 'include/segan_omlsa.h' in rule and '$(CSRC)/segan_stsa.h' in rule
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        doc = f.read()
    assert 'segan_omlsa.h' in doc and 'segan_omlsa_dims' in doc and 'segan_omlsa(' in doc
    # the existing rules and choices are as they were
    import clean
    from segan_pytorch_amd import baselines
    assert baselines.RULES == ('logmmse', 'wiener') and clean.BASELINES == ('wiener', 'logmmse')
    assert sorted(ops.DENOISE_RULES) == ['logmmse', 'wiener']


def test_dims_and_checks_before_any_launch():
    from segan_pytorch_amd import _lib, ops
    lib = _lib.load()
    for srate in (16000, 8000):
        F = srate // 50
        for L in (1, 6 * F - 1, 6 * F, 6 * F + F // 2 - 1, 6 * F + F // 2, 8000, 32000, 64000):
            nf = O.n_frames(L, srate)
            assert ops.omlsa_dims(3, L, srate) == dict(
                frame=F, hop=F // 2, nfft=2 * F, frames=nf,
                ws_bytes=3 * 16 * (F + 1) * max(nf, 1)), (L, srate)
    one = ctypes.c_void_p(16)     # never dereferenced: the arguments are refused first
    out = (ctypes.c_int64 * 5)()

    def call(x=one, xdt=0, rows=1, T=5000, srate=16000, y=one, ydt=2, nfr=one, ws=one):
        return lib.segan_omlsa(x, xdt, None, rows, T, srate, y, ydt, nfr, None, None, None, ws,
                               None)

    for rows, T, srate in ((0, 5000, 16000), (65536, 5000, 16000), (1, 0, 16000),
                           (1, (1 << 24) + 1, 16000), (1, 5000, 44100), (1, 5000, 0)):
        assert lib.segan_omlsa_dims(rows, T, srate, out) != 0
        assert lib.segan_last_error().startswith(b'omlsa: bad sizes')
        assert call(rows=rows, T=T, srate=srate) != 0
        assert lib.segan_last_error().startswith(b'omlsa: bad sizes')
        with pytest.raises(RuntimeError, match='omlsa: bad sizes'):
            ops.omlsa_dims(rows, T, srate)
    assert lib.segan_omlsa_dims(1, 5000, 16000, None) != 0
    assert lib.segan_last_error().startswith(b'omlsa: NULL')
    for kw in (dict(x=None), dict(y=None), dict(nfr=None), dict(ws=None)):
        assert call(**kw) != 0 and lib.segan_last_error().startswith(b'omlsa: NULL'), kw
    for kw in (dict(xdt=1), dict(ydt=1), dict(xdt=3), dict(ydt=-1)):
        assert call(**kw) != 0 and b'SEGAN_DT_F32' in lib.segan_last_error(), kw
        assert lib.segan_last_error().startswith(b'omlsa:')
    assert call(ws=ctypes.c_void_p(24)) != 0 and b'aligned' in lib.segan_last_error()
    assert lib.segan_last_error().startswith(b'omlsa:')


def test_cli_flags_leave_the_default_namespaces_alone():
    import clean
    import eval_noisy_performance as ev
    from segan_pytorch_amd import baselines
    p = clean.build_parser()
    assert sorted(vars(p.parse_args([]))) == sorted([
        'g_pretrained_ckpt', 'test_files', 'h5', 'seed', 'synthesis_path', 'cuda', 'soundfile',
        'cfg_file'])
    o = p.parse_args(['--omlsa', '--test_files', 'd'])
    assert o.omlsa is True and o.cfg_file is None and o.g_pretrained_ckpt is None
    assert baselines.omlsa_opts(o) is True and baselines.omlsa_opts(p.parse_args([])) is False
    assert baselines.omlsa_opts(p.parse_args(['--wpe', '--omlsa'])) is True
    with pytest.raises(SystemExit, match='baseline'):       # before any device is asked for
        clean.main(p.parse_args(['--omlsa', '--baseline', 'wiener', '--test_files', 'd']))
    with pytest.raises(SystemExit, match='cfg_file'):
        clean.main(p.parse_args(['--omlsa', '--cfg_file', 'c', '--test_files', 'd']))
    with pytest.raises(SystemExit, match='test_files'):     # --omlsa alone needs no checkpoint
        clean.main(p.parse_args(['--omlsa']))
    with pytest.raises(SystemExit, match='MI355X'):         # and gets as far as the device
        clean.main(p.parse_args(['--omlsa', '--test_files', 'd']))
    with pytest.raises(SystemExit, match='cfg_file'):       # without it the generator's needs hold
        clean.main(p.parse_args(['--test_files', 'd']))
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    base = parse()
    assert not hasattr(base, 'omlsa') and base.baseline is None
    assert parse('--omlsa').omlsa is True and baselines.omlsa_opts(parse('--omlsa'))
    for flags in ((), ('--stoi', '--sisdr'), ('--f0',)):
        assert ev.header_line(parse('--omlsa', *flags)) == ev.header_line(parse(*flags))
    assert ev.header_line(parse('--omlsa')) == 'FILE CSIG CBAK COVL PESQ SSNR'
    with pytest.raises(SystemExit, match='baseline'):
        ev.main(parse('--omlsa', '--baseline', 'logmmse'))
    with pytest.raises(SystemExit, match='baseline'):
        baselines.omlsa_opts(parse('--omlsa', '--baseline', 'wiener'))
    import argparse
    q = argparse.ArgumentParser()
    baselines.add_omlsa_flags(q)
    assert vars(q.parse_args([])) == {} and vars(q.parse_args(['--omlsa'])) == {'omlsa': True}


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import baselines, ops
    for x in (torch.zeros(2, 5000), torch.zeros(5000, dtype=torch.float64)):
        for fn in (ops.omlsa_rows, ops.omlsa_stages, baselines.omlsa):
            with pytest.raises(RuntimeError, match='MI355X'):
                fn(x)
    with pytest.raises(TypeError, match='omlsa_wav'):
        baselines.omlsa_wav(np.zeros((2, 100), np.float32))
    with pytest.raises(TypeError, match='omlsa_wav'):
        baselines.omlsa_wav(np.zeros(100, np.int32))


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['omlsa_rows', 'omlsa_stages'])
def test_ops_argument_checks_raise_before_any_launch(fn):
    from segan_pytorch_amd import ops
    f = getattr(ops, fn)
    x = _fake(2, 5000)
    with pytest.raises(TypeError, match='tensor'):
        f(np.zeros(5000, np.float32))
    for dt in (torch.float16, torch.int16, torch.complex128):
        with pytest.raises(TypeError, match='float32 or float64'):
            f(_fake(2, 5000, dtype=dt))
    with pytest.raises(ValueError, match=r'\[rows, T\] or \[T\]'):
        f(_fake(2, 2, 5000))
    with pytest.raises(ValueError, match='contiguous'):
        f(_fake(5000, 2).t())
    for bad in ([5000], [5000, 5001], [-1, 5000], [5000.0, 5000.0], [[5000, 5000]]):
        with pytest.raises(ValueError, match='lengths'):
            f(x, lengths=bad)
    for bad in (0, 44100, 16000.5, True, None):
        with pytest.raises(ValueError, match='srate'):
            f(x, srate=bad)
    for bad in (torch.float16, torch.int16, 'float32', 0):
        with pytest.raises(ValueError, match='out_dtype'):
            f(x, out_dtype=bad)
    for bad in (0, -1, 1.5, True, 1000):
        with pytest.raises(ValueError, match='ws_cap'):
            f(x, ws_cap=bad)
