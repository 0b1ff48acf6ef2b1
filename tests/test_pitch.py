"""Host side of the pitch tracker and the F0 / voicing measures (the numpy oracle
scripts/pitch_oracle.py, the fixture tests/golden/pitch.pt, the header, the CLI flags, the argument
checks of ops): no GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_pitch as GP  # noqa: E402
import pitch_oracle as O  # noqa: E402


@pytest.fixture(scope='module')
def pfx():
    return load_golden('pitch.pt')


def _glide(lo, hi, n, snr_db, seed):
    rng = np.random.default_rng(seed)
    f0 = np.geomspace(lo, hi, n)
    x = 0.3 * GP.harmonics(f0, 16000)
    if snr_db is not None:
        x = x + 10 ** (-snr_db / 20) * np.sqrt(np.mean(x ** 2)) * rng.standard_normal(n)
    return x.astype(np.float32), f0


def _frame_f0(f0, nf):
    """the true f0 at the middle of each frame's span of 400 + lag samples, about sample 80 t + 280"""
    return f0[np.minimum(80 * np.arange(nf) + 280, len(f0) - 1)]


def test_constants_and_frame_counts():
    assert O.constants(16000) == (80, 40, 266) and O.constants(8000) == (40, 20, 133)
    with pytest.raises(ValueError):
        O.constants(44100)
    got = [(O.n_blocks(L, 16000), O.n_frames(L, 16000)) for L in GP.LENGTHS]
    assert got == [(0, 0), (0, 0), (1, 0), (4, 0), (5, 1), (6, 2), (46, 42), (201, 197)]
    assert O.n_frames(333, 8000) == 0 and O.n_frames(334, 8000) == 1


@pytest.mark.parametrize('snr', [None, 40, 10])
def test_glides_have_no_gross_error_and_a_small_median_error(snr):
    for lo, hi in ((60.5, 120), (100, 400), (380, 150)):
        x, f0 = _glide(lo, hi, 12000, snr, 7)
        tr = O.track(x)
        v = tr['lag'] > 0
        assert v.mean() > 0.9, (lo, hi, snr, v.mean())
        rel = np.abs(tr['f0'][v] / _frame_f0(f0, len(v))[v] - 1.0)
        assert rel.max() < 0.2, (lo, hi, snr, rel.max())
        assert np.median(rel) < 0.01, (lo, hi, snr, np.median(rel))


def test_noise_silence_and_a_constant_are_unvoiced(pfx):
    noise = pfx['signals']['noise'].numpy()
    tr = O.track(noise)
    assert len(tr['lag']) == 197 and not tr['lag'].any() and not tr['f0'].any()
    assert (tr['ap'] > 0.15).all()
    for x in (np.zeros(3000, np.float32), np.full(3000, 0.25, np.float32)):
        tr = O.track(x)
        assert len(tr['lag']) == 30 and not tr['lag'].any() and not tr['f0'].any()
        assert (tr['ap'] == 1.0).all() and np.isinf(tr['margin']).all()
    # the gated signal: voiced where it is voiced, unvoiced in the silences and the noise burst
    sp = pfx['tracks']['speech@0.15']['lag'].numpy() > 0
    centre = 80 * np.arange(197) + 280
    assert not sp[centre < 1100].any() and not sp[(centre > 6500) & (centre < 7500)].any()
    assert sp[(centre > 2200) & (centre < 5500)].all() and sp[(centre > 8600) & (centre < 12500)].all()


def test_integer_periods_and_both_ends_of_the_lag_range():
    n = np.arange(4000)
    for period in (40, 41, 100, 177, 266):
        x = (0.4 * np.sin(2 * np.pi * n / period) + 0.2 * np.sin(4 * np.pi * n / period + 1.0))
        tr = O.track(x.astype(np.float32))
        assert (tr['lag'] == period).all(), (period, tr['lag'])
        assert np.abs(tr['f0'] * period / 16000.0 - 1.0).max() < 2e-3
    # tau_max is picked, with lag tau_max + 1 = 267 as the parabola's right neighbour
    tr = O.track((0.4 * np.sin(2 * np.pi * n / 266.4)).astype(np.float32))
    assert (tr['lag'] == 266).all() and (tr['f0'] < 16000 / 266.0).all()
    assert tr['cmnd'].shape[1] == 268
    # a period past the range: nothing below the threshold, or the descent stops at tau_max
    tr = O.track((0.4 * np.sin(2 * np.pi * n / 300.0)).astype(np.float32))
    assert np.isin(tr['lag'], (0, 266)).all()


def test_threshold_changes_decisions_and_is_checked(pfx):
    v = {th: int((pfx['tracks']['speech@{}'.format(th)]['lag'] > 0).sum()) for th in (0.1, 0.15, 0.3)}
    assert v[0.1] < v[0.15] < v[0.3]
    x = pfx['signals']['speech'].numpy()[:3000]
    for bad in (0, -0.1, 1.5):
        with pytest.raises(ValueError):
            O.track(x, theta=bad)
    assert len(O.track(x, theta=1.0)['lag']) == 30


def test_scaling_by_a_power_of_two_changes_nothing(pfx):
    x = pfx['signals']['glide'].numpy()[:4001]
    a, b = O.track(x), O.track((x * np.float32(2.0 ** -9)).astype(np.float32))
    for k in ('f0', 'lag', 'ap', 'cmnd'):
        assert np.array_equal(a[k], b[k]), k


def test_longdouble_agrees_on_every_decision(pfx):
    for name, srate in (('glide', 16000), ('speech', 16000), ('speech8', 8000)):
        x = pfx['signals'][name].numpy()[:6000]
        a, b = O.track(x, srate), O.track(x, srate, dtype=np.longdouble)
        assert np.array_equal(a['lag'], b['lag']) and b['f0'].dtype == np.longdouble
        v = a['lag'] > 0
        assert v.any() and np.abs(a['f0'][v] / b['f0'][v].astype(np.float64) - 1).max() < 1e-12


def test_measures_move_the_right_way_with_noise(pfx):
    e = pfx['evals']
    assert e['snr20']['f0_mae'] < e['snr10']['f0_mae'] < e['snr5']['f0_mae']
    assert e['snr20']['vuv_acc'] >= e['snr10']['vuv_acc'] > e['snr5']['vuv_acc']
    assert e['snr20']['f0_kld'] < e['snr10']['f0_kld'] < e['snr5']['f0_kld']
    assert math.isnan(e['noise']['f0_mae']) and math.isnan(e['noise']['f0_kld'])
    assert 0 < e['noise']['vuv_acc'] < 0.5
    assert all(abs(v['voiced'] - 127 / 197) < 1e-15 for v in e.values())
    t = pfx['tracks']['speech@0.15']
    same = O.f0_eval(t['f0'].numpy(), t['lag'].numpy(), t['f0'].numpy(), t['lag'].numpy())
    assert same['f0_mae'] == 0 and same['vuv_acc'] == 1 and abs(same['f0_kld']) < 1e-12


def test_contour_interpolates_in_the_log_domain():
    f0 = np.array([0, 0, 100.0, 0, 0, 0, 200.0, 0, 150.0, 0])
    lag = (f0 > 0).astype(np.int32) * 100
    l = O.contour(f0, lag)
    assert l[0] == l[1] == l[2] == np.log(100.0) and l[9] == np.log(150.0)
    assert np.allclose(l[3:6], np.log(100.0) + np.log(2.0) * np.array([1, 2, 3]) / 4, rtol=1e-15)
    assert abs(l[7] - 0.5 * (np.log(200.0) + np.log(150.0))) < 1e-15


def test_every_nan_rule():
    f = np.array([100.0, 0, 110.0, 120.0])
    lg = np.array([160, 0, 145, 133], np.int32)
    z, zl = np.zeros(4), np.zeros(4, np.int32)
    e = O.f0_eval(f[:0], lg[:0], f[:0], lg[:0])
    assert all(math.isnan(v) for v in e.values())
    e = O.f0_eval(z, zl, f, lg)             # no voiced frame in ref
    assert math.isnan(e['f0_mae']) and math.isnan(e['f0_kld'])
    assert e['vuv_acc'] == 0.25 and e['voiced'] == 0
    e = O.f0_eval(f, lg, z, zl)             # none in deg
    assert math.isnan(e['f0_mae']) and math.isnan(e['f0_kld'])
    assert e['vuv_acc'] == 0.25 and e['voiced'] == 0.75
    e = O.f0_eval(f[:1], lg[:1], f[:1], lg[:1])      # one frame
    assert e['f0_mae'] == 0 and e['vuv_acc'] == 1 and math.isnan(e['f0_kld'])
    c = np.array([100.0, 0, 0, 100.0])
    e = O.f0_eval(f, lg, c, (c > 0).astype(np.int32))    # a constant processed contour
    assert math.isfinite(e['f0_mae']) and math.isnan(e['f0_kld']) and e['vuv_acc'] == 0.75
    e = O.f0_eval(c, (c > 0).astype(np.int32), f, lg)    # a constant reference: the literal formula
    assert not math.isnan(e['f0_kld'])
    e = O.f0_eval(f, lg, f * 1.1, lg)
    assert abs(e['f0_mae'] - 11.0) < 1e-9 and e['vuv_acc'] == 1
    assert abs(e['f0_kld'] - np.log(1.1) ** 2 / (2 * np.var(O.contour(f, lg), ddof=1))) < 1e-9


def test_fixture_margins_tolerances_and_size(pfx):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'pitch.pt'))
    assert size < 1024 * 1024, size
    meta = pfx['meta']
    assert meta['margin_floor'] == 1e-7 and meta['min_margin'] >= 1e-7
    assert pfx['lengths'] == [0, 266, 347, 666, 667, 747, 4001, 16384]
    for k in ('cmnd', 'ap', 'f0', 'f0_mae', 'f0_kld'):
        assert 0 <= meta['gaps'][k] and 100 * meta['gaps'][k] <= 1e-10, k
    # the rounding of d' that the margin has to cover: orders of magnitude below it
    assert 100 * meta['gaps']['cmnd'] * 1e3 < meta['min_margin']
    assert [len(pfx['ragged'][L]['lag']) for L in pfx['lengths']] == [0, 0, 0, 0, 1, 2, 42, 197]
    assert 'cmnd' in pfx['ragged'][4001] and 'cmnd' not in pfx['ragged'][16384]
    assert pfx['ragged'][4001]['cmnd'].shape == (42, 268)
    assert pfx['tracks']['speech8_short']['cmnd'].shape == (17, 135)
    for s in pfx['signals'].values():
        assert s.dtype == torch.float32


def test_regenerating_a_small_case_reproduces_the_fixture_bits(pfx):
    x = pfx['signals']['glide'].numpy()
    for L in (667, 747, 4001):
        tr, want = O.track(x[:L]), pfx['ragged'][L]
        for k in ('f0', 'lag', 'ap', 'cmnd', 'scale'):
            assert np.array_equal(tr[k], want[k].numpy()), (L, k)
        assert tr['margin'].min() >= pfx['meta']['min_margin']
    tr = O.track(pfx['signals']['speech8'].numpy()[:GP.N8_SHORT], 8000)
    assert np.array_equal(tr['cmnd'], pfx['tracks']['speech8_short']['cmnd'].numpy())
    deg = GP.processed({k: v.numpy() for k, v in pfx['signals'].items()}, pfx['gains'])
    assert np.array_equal(O.track(deg['snr10'])['lag'], pfx['tracks']['snr10']['lag'].numpy())


def test_abi_header_and_makefile_pins():
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    block = H.RAW[H.RAW.index('Pitch tracking by YIN'):H.RAW.index('int segan_pitch_frames')]
    assert 'Added\n * without a change of SEGAN_ABI_VERSION: the exports are purely additive.' in block
    assert H.macro('SEGAN_PITCH_NB') == ops.PITCH_NB and ops.PITCH_NB == O.NB == 5
    for name, nargs in (('segan_pitch_frames', 2), ('segan_pitch_dims', 4), ('segan_pitch', 11),
                        ('segan_pitch_cmnd', 8), ('segan_f0_eval', 9)):
        assert len(H.args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert '$(CSRC)/segan_pitch.hip' in mk.split('SRCS :=')[1].split('\n')[0]
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(n in doc for n in ('segan_pitch_dims', 'segan_pitch_cmnd', 'segan_f0_eval'))
    lib = _lib.load()
    assert lib.segan_abi_version() == 17


def test_dims_frames_and_checks_before_any_launch():
    import ctypes
    from segan_pytorch_amd import _lib, ops
    lib = _lib.load()
    for srate in (16000, 8000):
        for L in (0, 133, 134, 266, 267, 333, 334, 347, 666, 667, 747, 4001, 16384):
            assert lib.segan_pitch_frames(L, srate) == O.n_frames(L, srate), (L, srate)
    assert lib.segan_pitch_frames(16384, 16000) == 197
    assert lib.segan_pitch_frames(1000, 44100) == -1
    assert lib.segan_last_error().startswith(b'pitch:')
    assert ops.pitch_dims(3, 16384) == dict(hop=80, tau_min=40, tau_max=266, blocks=201,
                                            frames=197, ws_doubles=3 * 201 * 2 * 268)
    assert ops.pitch_dims(1, 666)['frames'] == 0 and ops.pitch_dims(1, 266)['ws_doubles'] == 0
    d8 = ops.pitch_dims(1, 6000, 8000)
    assert (d8['hop'], d8['tau_min'], d8['tau_max'], d8['frames']) == (40, 20, 133, 142)
    one = ctypes.c_void_p(16)     # never dereferenced: the arguments are refused first
    out = (ctypes.c_int64 * 6)()
    for rows, T, srate in ((0, 5000, 16000), (65536, 5000, 16000), (1, 0, 16000),
                           (1, (1 << 24) + 1, 16000), (1, 5000, 44100), (1, 5000, 0)):
        assert lib.segan_pitch_dims(rows, T, srate, out) != 0
        assert lib.segan_pitch(one, None, rows, T, srate, 0.15, one, one, one, one, None) != 0
        assert lib.segan_last_error().startswith(b'pitch:')
        assert lib.segan_pitch_cmnd(one, None, rows, T, srate, one, one, None) != 0
    for theta in (0.0, -1.0, 1.5, float('nan')):
        assert lib.segan_pitch(one, None, 1, 5000, 16000, theta, one, one, one, one, None) != 0
        assert b'threshold' in lib.segan_last_error()
    assert lib.segan_pitch(None, None, 1, 5000, 16000, 0.15, one, one, one, one, None) != 0
    assert lib.segan_f0_eval(None, one, one, one, None, 1, 5, one, None) != 0
    assert lib.segan_last_error().startswith(b'f0_eval:')
    for rows, F in ((0, 5), (65536, 5), (1, -1)):
        assert lib.segan_f0_eval(one, one, one, one, None, rows, F, one, None) != 0


def test_eval_cli_flag_leaves_every_old_header_line_alone():
    import itertools
    import eval_noisy_performance as ev
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    assert parse().f0 is False and parse('--f0').f0 is True
    assert ev.EXTRA == (('STOI', 'stoi', 'stoi'), ('ESTOI', 'estoi', 'estoi'),
                        ('FWSEGSNR', 'fwsegsnr', 'fwsegsnr'), ('CD', 'cd', 'cepstral_distance'),
                        ('SISDR', 'sisdr', 'si_sdr'), ('SDR', 'sdr', 'sdr'),
                        ('SRMR', 'srmr', 'srmr'))
    assert ev.BLIND == ('SRMR',)
    assert ev.F0_COLUMNS == (('F0MAE', 'f0_mae'), ('VUV', 'vuv_acc'), ('F0KLD', 'f0_kld'))
    names = ['STOI', 'ESTOI', 'FWSEGSNR', 'CD', 'SISDR', 'SDR', 'SRMR']
    flags = ['--stoi', '--estoi', '--fwsegsnr', '--cd', '--sisdr', '--sdr', '--srmr']
    for on in itertools.product((False, True), repeat=7):
        old = 'FILE CSIG CBAK COVL PESQ SSNR' + ''.join(' ' + n for n, o in zip(names, on) if o)
        chosen = [f for f, o in zip(flags, on) if o]
        assert ev.header_line(parse(*chosen)) == old
        assert ev.header_line(parse('--f0', *chosen)) == old + ' F0MAE VUV F0KLD'


def test_train_parses_the_flag():
    import train
    assert train.build_parser().parse_args([]).eval_f0 is False
    o = train.build_parser().parse_args(['--eval_f0'])
    assert o.eval_f0 is True and o.eval_srmr is False


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import ops, quality
    x = torch.zeros(2, 5000)
    for fn in (ops.pitch, ops.pitch_stages, quality.pitch):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x)
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.f0_eval(x, x)
    f, l = torch.zeros(2, 5, dtype=torch.float64), torch.zeros(2, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.f0_eval(f, l, f, l)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['pitch', 'pitch_stages'])
def test_ops_argument_checks_raise_before_any_launch(fn):
    from segan_pytorch_amd import ops
    f = getattr(ops, fn)
    x = _fake(2, 5000)
    with pytest.raises(ValueError, match='2 dims'):
        f(_fake(2, 5000)[0])
    with pytest.raises(TypeError, match='float32'):
        f(_fake(2, 5000, dtype=torch.float64))
    for bad in ([5000], [5000, 5001], [-1, 5000], [5000.0, 5000.0], [[5000, 5000]]):
        with pytest.raises(ValueError, match='lengths'):
            f(x, lengths=bad)
    for bad in (0, 44100, 16000.5, True, None):
        with pytest.raises(ValueError, match='srate'):
            f(x, srate=bad)
    for bad in (0, 0.0, -0.1, 1.01, True, None, '0.15', float('nan')):
        with pytest.raises(ValueError, match='threshold'):
            f(x, threshold=bad)
    for bad in (0, -1, 1.5, True, 1000):
        with pytest.raises(ValueError, match='ws_cap'):
            f(x, ws_cap=bad)


def test_f0_eval_argument_checks():
    from segan_pytorch_amd import ops, quality
    f, l = _fake(2, 5, dtype=torch.float64), _fake(2, 5, dtype=torch.int32)
    with pytest.raises(TypeError, match='float64'):
        ops.f0_eval(_fake(2, 5), l, f, l)
    with pytest.raises(TypeError, match='int32'):
        ops.f0_eval(f, _fake(2, 5, dtype=torch.int64), f, l)
    with pytest.raises(ValueError, match='shapes'):
        ops.f0_eval(f, l, _fake(2, 6, dtype=torch.float64), l)
    with pytest.raises(ValueError, match='nframes'):
        ops.f0_eval(f, l, f, l, nframes=_fake(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='differ in shape'):
        quality.f0_eval(_fake(2, 5000), _fake(2, 5001))
