"""Host side of the BSS-eval SDR (the numpy oracle scripts/sdr_oracle.py, the fixture
tests/golden/sdr.pt, the header, the CLI flags, the argument checks of ops): no GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_sdr as GS  # noqa: E402
import sdr_oracle as O  # noqa: E402


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


@pytest.fixture(scope='module')
def sfx():
    return load_golden('sdr.pt')


def _toeplitz(r):
    n = len(r)
    return np.asarray(r)[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])]


def test_one_tap_is_the_closed_form(qfx):
    for name in ('snr10', 'filtered', 'short'):
        ref, deg = GS.case_signals(qfx, name)
        s, x = ref.astype(np.float64), deg.astype(np.float64)
        alpha = np.dot(s, x) / np.dot(s, s)
        e = x - alpha * s
        want = 10 * math.log10(alpha ** 2 * np.dot(s, s) / np.dot(e, e))
        assert abs(O.sdr(ref, deg, 1) - want) <= 1e-10, name
        assert abs(O.sdr_one_tap(ref, deg) - want) <= 1e-10, name


def test_exact_copies_are_inf_and_silence_is_nan(qfx):
    ref, deg = GS.case_signals(qfx, 'snr10')
    ref, deg = ref[:3000], deg[:3000]
    for taps in (1, 33, 512):
        assert O.sdr(ref, ref, taps) == math.inf
        assert O.sdr(ref, (0.5 * ref).astype(np.float32), taps) == math.inf
        st = O.sdr_stages(ref, (0.5 * ref).astype(np.float32), taps)
        assert st['order'] == taps and st['c'][0] == 0.5 and not st['c'][1:].any()
        assert math.isnan(O.sdr(np.zeros_like(ref), deg, taps))
        assert math.isnan(O.sdr(ref, np.zeros_like(deg), taps))
        assert math.isnan(O.sdr(ref[:0], deg[:0], taps))
    with pytest.raises(ValueError):
        O.sdr(ref, deg, 513)
    with pytest.raises(ValueError):
        O.sdr(ref, deg, 0)


def test_power_of_two_gain_scales_the_cross_correlation_bit_for_bit(qfx):
    ref, _ = GS.case_signals(qfx, 'snr10')
    r, d = O.correlations(ref, (0.25 * ref).astype(np.float32), 64)
    assert np.array_equal(d, 0.25 * r)


def test_sdr_is_monotone_in_snr_and_the_filter_is_found(qfx, sfx):
    for taps in (1, 33):
        v = [O.sdr(*GS.case_signals(qfx, n), taps) for n in ('snr0', 'snr10', 'snr20')]
        assert v[0] < v[1] < v[2], (taps, v)
    res = sfx['results']
    for taps in sfx['taps']:
        assert res['snr0'][taps]['sdr'] < res['snr10'][taps]['sdr'] < res['snr20'][taps]['sdr']
    assert res['filtered'][512]['sdr'] > res['filtered'][1]['sdr'] + 3.0
    c = res['filtered'][512]['c'].numpy()
    assert np.abs(c[[0, 7, 39]] - np.array([1.0, 0.5, -0.3])).max() < 0.05


def test_lags_past_the_length_are_zero(qfx):
    ref, deg = GS.case_signals(qfx, 'tiny')
    st = O.sdr_stages(ref[:20], deg[:20], 33)
    assert not st['r'][20:].any() and not st['d'][20:].any() and st['r'][19] != 0.0
    assert st['order'] == 33 and math.isfinite(st['sdr'])


def test_recursion_solves_the_normal_equations(qfx):
    ref, deg = GS.case_signals(qfx, 'snr10')
    for n in (1, 2, 33, 512):
        r, d = O.correlations(ref, deg, n)
        c, order = O.levinson(r, d)
        assert order == n
        assert np.abs(_toeplitz(r) @ c - d).max() <= 1e-9 * r[0]
        assert np.abs(c - O.solve_lstsq(r, d)).max() <= 1e-6 * np.abs(c).max()


def test_guard_stops_a_rank_two_system_at_order_two():
    r = np.cos(0.3 * np.arange(64))
    c, order = O.levinson(r, r.copy())
    assert order == 2 and not c[2:].any()
    assert np.abs(_toeplitz(r) @ c - r).max() <= 1e-12
    c0, order0 = O.levinson(np.zeros(8), np.ones(8))
    assert order0 == 0 and not c0.any()


def test_recipe_reproduces_the_fixture(qfx, sfx):
    assert sfx['cases'] == GS.CASES and tuple(sfx['taps']) == GS.TAPS == (1, 2, 33, 512)
    assert all(rc['len'] <= 3 * 4096 for rc in GS.CASES.values())
    for name in GS.CASES:
        ref, deg = GS.case_signals(qfx, name)
        assert ref.dtype == deg.dtype == np.float32 and len(ref) == GS.CASES[name]['len']
        for taps in (1, 33):
            got, want = GS.evaluate(ref, deg, taps), sfx['results'][name][taps]
            assert abs(got['sdr'] - want['sdr']) <= 1e-11, (name, taps)
            for k in ('r', 'd'):
                assert np.abs(got[k] - want[k].numpy()).max() <= 1e-12 * got['r'][0], (name, k)
            for k in ('target_energy', 'error_energy'):
                assert abs(got[k] - want[k]) <= 1e-11 * want[k], (name, k)
    ref, _ = GS.case_signals(qfx, 'zero_run')
    assert not ref[4000:6000].any() and ref[3999] != 0 and ref[6000] != 0


def test_fixture_is_small_stores_no_signals_and_bounds_the_tolerance(sfx):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'sdr.pt'))
    assert size < 256 * 1024, size
    meta = sfx['meta']
    assert 'signals' not in sfx and meta['signals'] == 'tests/golden/quality.pt'
    assert 0 <= meta['solver_gap_db'] < 1e-10
    assert 0 <= meta['definition_gap_db'] < 1e-8
    for name, per in sfx['results'].items():
        for taps, r in per.items():
            assert math.isfinite(r['sdr']) and r['sdr'] < 60.0, (name, taps)
            assert r['order'] == taps and r['r'].shape == r['d'].shape == r['c'].shape == (taps,)


def test_abi_entries_are_additive():
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    assert re.search(r'\bint segan_sdr_dims\(int rows, int T, int taps, long long\* out\);', H.CODE)
    assert re.search(r'\bint segan_sdr\(const float\* ref, const float\* deg, const int\* lengths, '
                     r'int rows, int T, int taps,\s+double\* row_out, double\* stages_out, '
                     r'double\* ws, void\* stream\);', H.CODE)
    assert re.search(r'\bint segan_toeplitz_solve\(const double\* r, const double\* d, int rows, '
                     r'int n, double\* c_out,\s+int\* order_out, void\* stream\);', H.CODE)
    for name, nargs in (('segan_sdr_dims', 4), ('segan_sdr', 10), ('segan_toeplitz_solve', 7)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
    assert H.macro('SEGAN_SDR_SPAN') == ops.SDR_SPAN
    assert H.macro('SEGAN_SDR_MAX_TAPS') == ops.SDR_TAPS and ops.SDR_TAPS == 512
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    # arguments are checked before any launch: no device is needed to be refused
    assert lib.segan_sdr(None, None, None, 1, 4000, 512, None, None, None, None) != 0
    assert b'sdr' in lib.segan_last_error()
    assert lib.segan_toeplitz_solve(None, None, 1, 8, None, None, None) != 0
    assert b'toeplitz_solve' in lib.segan_last_error()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(n in doc for n in ('segan_sdr_dims', 'segan_sdr', 'segan_toeplitz_solve'))


def test_sdr_dims_and_size_checks():
    import ctypes
    from segan_pytorch_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 3)()
    assert lib.segan_sdr_dims(5, 2 * 4096 + 17, 33, out) == 0
    # [rows][nspans][2 taps] + [rows][ceil((T + taps - 1) / span)][2] + [rows][3 taps + 3]
    assert list(out) == [4096, 3, 5 * (3 * 66 + 3 * 2 + 102)]
    assert lib.segan_sdr_dims(1, 4096, 2, out) == 0 and list(out)[1:] == [1, 4 + 4 + 9]
    for rows, T, taps in ((0, 100, 8), (65536, 100, 8), (1, 0, 8), (1, 100, 0), (1, 100, 513)):
        assert lib.segan_sdr_dims(rows, T, taps, out) != 0, (rows, T, taps)
        assert b'sdr:' in lib.segan_last_error()
    one = ctypes.c_void_p(8)     # never dereferenced: the sizes are refused first
    for rows, n in ((0, 8), (65536, 8), (1, 0), (1, 513)):
        assert lib.segan_toeplitz_solve(one, one, rows, n, one, one, None) != 0
        assert b'toeplitz_solve:' in lib.segan_last_error()
    for rows, T, taps in ((0, 100, 8), (1, 0, 8), (1, 100, 0), (1, 100, 513)):
        assert lib.segan_sdr(one, one, None, rows, T, taps, one, None, one, None) != 0
        assert b'sdr:' in lib.segan_last_error()


def test_eval_cli_flag_and_unchanged_header_line():
    import eval_noisy_performance as ev
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    assert parse().sdr is False and parse('--sdr').sdr is True
    assert ev.header_line(parse()) == 'FILE CSIG CBAK COVL PESQ SSNR'
    assert ev.header_line(parse('--sisdr')) == 'FILE CSIG CBAK COVL PESQ SSNR SISDR'
    assert ev.header_line(parse('--sdr', '--sisdr')).endswith(' SISDR SDR')
    assert ev.header_line(parse('--sdr', '--stoi')) == 'FILE CSIG CBAK COVL PESQ SSNR STOI SDR'


def test_train_parses_the_eval_flag():
    import train
    assert train.build_parser().parse_args([]).eval_sdr is False
    o = train.build_parser().parse_args(['--eval_sdr'])
    assert o.eval_sdr is True and o.eval_sisdr is False


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import ops, quality
    x = torch.zeros(2, 4000)
    for fn in (ops.sdr, ops.sdr_stages, quality.sdr):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x, x)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.toeplitz_solve(x.double(), x.double())


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(rows, T, dtype=torch.float32):
    return torch.zeros(rows, T, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['sdr', 'sdr_stages'])
def test_ops_argument_checks_raise_before_any_launch(fn):
    from segan_pytorch_amd import ops
    f = getattr(ops, fn)
    x = _fake(2, 4000)
    with pytest.raises(ValueError, match='shapes differ'):
        f(x, _fake(2, 3999))
    with pytest.raises(ValueError, match='2 dims'):
        f(_fake(2, 4000)[0], _fake(2, 4000)[0])
    with pytest.raises(TypeError, match='float32'):
        f(_fake(2, 4000, torch.float64), _fake(2, 4000, torch.float64))
    for bad in ([4000], [4000, 4001], [-1, 4000], [4000.0, 4000.0], [[4000, 4000]], [True, False]):
        with pytest.raises(ValueError, match='lengths'):
            f(x, x, lengths=bad)
    for bad in (0, 513, -1, 33.0, True):
        with pytest.raises(ValueError, match='taps'):
            f(x, x, taps=bad)


def test_toeplitz_solve_argument_checks():
    from segan_pytorch_amd import ops
    r = _fake(2, 64, torch.float64)
    with pytest.raises(TypeError, match='float64'):
        ops.toeplitz_solve(_fake(2, 64), _fake(2, 64))
    with pytest.raises(ValueError, match='one shape'):
        ops.toeplitz_solve(r, _fake(2, 63, torch.float64))
    with pytest.raises(ValueError, match='1 .. 512'):
        ops.toeplitz_solve(_fake(2, 513, torch.float64), _fake(2, 513, torch.float64))
    with pytest.raises(TypeError, match='tensor'):
        ops.toeplitz_solve([1.0], [1.0])
