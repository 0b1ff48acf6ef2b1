"""Host side of SRMR (the numpy / scipy oracle scripts/srmr_oracle.py, the fixture
tests/golden/srmr.pt, the header, the CLI flags, the argument checks of ops): no GPU."""
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
import make_golden_srmr as GS  # noqa: E402
import srmr_oracle as O  # noqa: E402


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


@pytest.fixture(scope='module')
def sfx():
    return load_golden('srmr.pt')


def _response(b, a, f, fs):
    zi = np.exp(-2j * np.pi * np.asarray(f, dtype=np.float64) / fs)
    return (b[0] + b[1] * zi + b[2] * zi * zi) / (a[0] + a[1] * zi + a[2] * zi * zi)


@pytest.mark.parametrize('fs', [8000, 16000])
def test_gammatone_cascade_has_unit_gain_at_its_centre_frequency(fs):
    b, a, gain = O.gammatone_sections(fs)
    cfs = O.centre_freqs(fs)
    assert len(cfs) == 23 and np.all(np.diff(cfs) < 0) and abs(cfs[-1] - 125.0) < 1e-9
    assert cfs[0] < fs / 2
    for i, cf in enumerate(cfs):
        h = np.prod([_response(b[i, j], a[i], cf, fs) for j in range(4)])
        assert abs(abs(h) - 1.0) <= 1e-10, (i, abs(h))
    assert np.abs(gain / O.slaney_gain(fs) - 1.0).max() <= 1e-10


@pytest.mark.parametrize('fs', [8000, 16000])
def test_modulation_biquad_peaks_at_its_centre(fs):
    b, a, cutoffs = O.modulation_sections(fs)
    f = O.modulation_centres()
    assert abs(f[0] - 4.0) < 1e-12 and abs(f[7] - 128.0) < 1e-9
    for k in range(8):
        grid = f[k] * np.linspace(0.5, 2.0, 3001)
        mag = np.abs(_response(b[k], a[k], grid, fs))
        assert abs(grid[np.argmax(mag)] / f[k] - 1.0) < 2e-3, k
        assert abs(abs(_response(b[k], a[k], f[k], fs)) - 1.0) <= 1e-12, k
        assert cutoffs[k] < f[k]
    assert np.all(np.diff(cutoffs) > 0)


def test_frames_are_full_frames_only():
    assert O.frame_sizes(16000) == (4096, 1024) and O.frame_sizes(8000) == (2048, 512)
    assert [O.n_frames(n, 16000) for n in (4095, 4096, 5119, 5120, 12305)] == [0, 1, 1, 2, 9]
    w = O.hamming_periodic(4096)
    assert abs(w[0] - 0.08) < 1e-15 and abs(w[2048] - 1.0) < 1e-15 and w[1] == w[4095]


def test_scale_invariance_and_the_nan_rows(qfx):
    x = GS.case_signal(qfx, 'n4097')
    a, b = O.stages(x), O.stages((0.25 * x).astype(np.float32))
    assert a['srmr'] == b['srmr'] and a['bw'] == b['bw'] and a['kstar'] == b['kstar']
    assert np.array_equal(a['energy'] * 0.0625, b['energy'])
    assert math.isnan(O.srmr(x[:4095])) and O.stages(x[:4095])['kstar'] == 0
    assert math.isnan(O.srmr(np.zeros(5000, np.float32)))
    assert math.isnan(O.srmr(x[:0]))
    with pytest.raises(ValueError):
        O.srmr(x, 44100)


def test_kstar_rule():
    c = O.modulation_sections(16000)[2]
    mid = lambda i: 0.5 * (c[i] + c[i + 1])  # noqa: E731
    assert [O.kstar_of(v, c) for v in (mid(4), mid(5), mid(6), c[7] + 1)] == [5, 6, 7, 8]
    assert O.kstar_of(c[4], c) == 5 and O.kstar_of(c[4] - 1, c) == 5    # the undefined range


def test_recipe_reproduces_the_fixture(qfx, sfx):
    assert sfx['cases'] == GS.CASES and sfx['rate'] == GS.RATE == 16000 and sfx['rir'] == GS.RIR
    assert set(GS.CASES) == {'dry', 'reverberant', 'snr0', 'snr20', 'n4096', 'n4097'}
    assert GS.CASES['n4096']['len'] == 4096 and GS.CASES['n4097']['len'] == 4097
    for name in ('reverberant', 'n4096', 'n4097'):
        x = GS.case_signal(qfx, name)
        assert x.dtype == np.float32 and len(x) == GS.CASES[name]['len'] <= 12305
        got, want = GS.evaluate(x), sfx['results'][name]
        assert abs(got['srmr'] - want['srmr']) <= 1e-11 * want['srmr'], name
        assert got['kstar'] == want['kstar'] and got['bw'] == want['bw']
        assert np.array_equal(got['cfs'], want['cfs'].numpy())
        for k in ('energy', 'envelope_energy'):
            w = want[k].numpy()
            assert np.abs(got[k] - w).max() <= 1e-11 * w.max(), (name, k)
    h = GS.impulse_response()
    assert h[0] == 1.0 and len(h) == GS.RIR['taps'] and np.abs(h[-100:]).max() < 1e-2


def test_fixture_is_small_stores_no_signals_and_bounds_the_tolerance(sfx):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'srmr.pt'))
    assert size < 256 * 1024, size
    meta = sfx['meta']
    assert 'signals' not in sfx and meta['signals'] == 'tests/golden/quality.pt'
    assert 0 <= meta['oracle_gap'] and 100 * meta['oracle_gap'] <= 1e-8
    assert 0 <= meta['definition_gap'] < 0.1
    res = sfx['results']
    assert res['reverberant']['srmr'] < res['dry']['srmr']
    assert res['snr0']['srmr'] < res['snr20']['srmr']
    for name, r in res.items():
        assert math.isfinite(r['srmr']) and r['srmr'] > 0, name
        assert abs(r['share'] - 90.0) > meta['share_margin'] >= 1e-6, name
        assert r['kstar'] in (5, 6, 7, 8) and r['energy'].shape == (23, 8)
        assert r['envelope_energy'].shape == r['cfs'].shape == (23,)


def test_abi_entries_are_additive():
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    assert re.search(r'\bint segan_fft_z2z\(const double\* in, double\* out, int rows, int log2n, '
                     r'int inverse,\s+void\* stream\);', H.CODE)
    assert re.search(r'\bint segan_srmr_dims\(int rows, int T, int rate, long long\* out\);', H.CODE)
    assert re.search(r'\bint segan_srmr\(const float\* x, const int\* lengths, int rows, int T, '
                     r'int rate,\s+double\* row_out,\s+double\* stages_out, double\* ws, '
                     r'void\* stream\);', H.CODE)
    for name, nargs in (('segan_fft_z2z', 6), ('segan_srmr_dims', 4), ('segan_srmr', 9)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
    for macro, value in (('SEGAN_SRMR_CHANNELS', ops.SRMR_CHANNELS),
                         ('SEGAN_SRMR_BANDS', ops.SRMR_BANDS), ('SEGAN_SRMR_STAGE', ops.SRMR_STAGE),
                         ('SEGAN_FFT_LDS_LOG2', ops.FFT_LDS_LOG2),
                         ('SEGAN_FFT_MAX_LOG2', ops.FFT_MAX_LOG2)):
        assert H.macro(macro) == value
    assert (ops.SRMR_CHANNELS, ops.SRMR_BANDS, ops.FFT_MAX_LOG2) == (23, 8, 20)
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    # arguments are checked before any launch: no device is needed to be refused
    assert lib.segan_srmr(None, None, 1, 5000, 16000, None, None, None, None) != 0
    assert lib.segan_last_error().startswith(b'srmr:')
    assert lib.segan_fft_z2z(None, None, 1, 4, 0, None) != 0
    assert lib.segan_last_error().startswith(b'fft:')
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(n in doc for n in ('segan_fft_z2z', 'segan_srmr_dims', 'segan_srmr'))


def test_srmr_dims_and_size_checks():
    import ctypes
    from segan_pytorch_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 4)()
    assert lib.segan_srmr_dims(5, 12305, 16000, out) == 0
    # Y [23][L] complex + E [23][8][frames] + envelope energies [23] + the stage block
    per = 2 * 23 * 16384 + 184 * 9 + 23 + 234
    assert list(out) == [16384, 9, per, 5 * per]
    assert lib.segan_srmr_dims(1, 4096, 16000, out) == 0 and list(out)[:2] == [4096, 1]
    assert lib.segan_srmr_dims(1, 4097, 16000, out) == 0 and list(out)[:2] == [8192, 1]
    assert lib.segan_srmr_dims(1, 5120, 16000, out) == 0 and list(out)[:2] == [8192, 2]
    assert lib.segan_srmr_dims(1, 4095, 16000, out) == 0 and list(out)[:2] == [4096, 0]
    assert lib.segan_srmr_dims(1, 4095, 8000, out) == 0 and list(out)[:2] == [4096, 4]
    assert lib.segan_srmr_dims(2, 1 << 20, 16000, out) == 0 and list(out)[0] == 1 << 20
    one = ctypes.c_void_p(16)     # never dereferenced: the sizes are refused first
    for rows, T, rate in ((0, 5000, 16000), (65536, 5000, 16000), (1, 0, 16000),
                          (1, (1 << 20) + 1, 16000), (1, 5000, 44100), (1, 5000, 0)):
        assert lib.segan_srmr_dims(rows, T, rate, out) != 0, (rows, T, rate)
        assert lib.segan_last_error().startswith(b'srmr:')
        assert lib.segan_srmr(one, None, rows, T, rate, one, None, one, None) != 0
        assert lib.segan_last_error().startswith(b'srmr:')
    assert lib.segan_srmr(one, None, 1, 5000, 16000, one, None, ctypes.c_void_p(8), None) != 0
    assert b'aligned' in lib.segan_last_error()
    for rows, lg in ((0, 4), (65536, 4), (1, 0), (1, 21)):
        assert lib.segan_fft_z2z(one, one, rows, lg, 0, None) != 0
        assert lib.segan_last_error().startswith(b'fft:')
    assert lib.segan_fft_z2z(one, one, 1, 13, 0, None) != 0      # two levels: not in place
    assert b'in place' in lib.segan_last_error()
    assert lib.segan_fft_z2z(ctypes.c_void_p(8), one, 1, 4, 0, None) != 0
    assert b'aligned' in lib.segan_last_error()


def test_eval_cli_flag_and_unchanged_header_lines():
    import eval_noisy_performance as ev
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    assert parse().srmr is False and parse('--srmr').srmr is True
    assert ev.header_line(parse()) == 'FILE CSIG CBAK COVL PESQ SSNR'
    assert ev.header_line(parse('--sisdr')) == 'FILE CSIG CBAK COVL PESQ SSNR SISDR'
    assert ev.header_line(parse('--sdr', '--stoi')) == 'FILE CSIG CBAK COVL PESQ SSNR STOI SDR'
    assert ev.header_line(parse('--stoi', '--estoi', '--fwsegsnr', '--cd', '--sisdr', '--sdr')) == (
        'FILE CSIG CBAK COVL PESQ SSNR STOI ESTOI FWSEGSNR CD SISDR SDR')
    assert ev.header_line(parse('--srmr')) == 'FILE CSIG CBAK COVL PESQ SSNR SRMR'
    assert ev.header_line(parse('--srmr', '--sdr', '--stoi')).endswith(' STOI SDR SRMR')
    assert ev.EXTRA[:6] == (('STOI', 'stoi', 'stoi'), ('ESTOI', 'estoi', 'estoi'),
                            ('FWSEGSNR', 'fwsegsnr', 'fwsegsnr'), ('CD', 'cd', 'cepstral_distance'),
                            ('SISDR', 'sisdr', 'si_sdr'), ('SDR', 'sdr', 'sdr'))
    assert ev.EXTRA[6:] == (('SRMR', 'srmr', 'srmr'),) and ev.BLIND == ('SRMR',)


def test_train_and_clean_parse_the_flags():
    import clean
    import train
    assert train.build_parser().parse_args([]).eval_srmr is False
    o = train.build_parser().parse_args(['--eval_srmr'])
    assert o.eval_srmr is True and o.eval_sdr is False
    assert not hasattr(clean.build_parser().parse_args([]), 'srmr')
    assert clean.build_parser().parse_args(['--srmr']).srmr is True


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import ops, quality
    x = torch.zeros(2, 5000)
    for fn in (ops.srmr, ops.srmr_stages, quality.srmr):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.fft_pow2(torch.zeros(2, 8, dtype=torch.complex128))


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(rows, T, dtype=torch.float32):
    return torch.zeros(rows, T, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['srmr', 'srmr_stages'])
def test_ops_argument_checks_raise_before_any_launch(fn):
    from segan_pytorch_amd import ops
    f = getattr(ops, fn)
    x = _fake(2, 5000)
    with pytest.raises(ValueError, match='2 dims'):
        f(_fake(2, 5000)[0])
    with pytest.raises(TypeError, match='float32'):
        f(_fake(2, 5000, torch.float64))
    for bad in ([5000], [5000, 5001], [-1, 5000], [5000.0, 5000.0], [[5000, 5000]], [True, False]):
        with pytest.raises(ValueError, match='lengths'):
            f(x, lengths=bad)
    for bad in (0, 44100, 16000.5, True, None):
        with pytest.raises(ValueError, match='rate'):
            f(x, rate=bad)
    for bad in (0, -1, 1.5, True, 1000):
        with pytest.raises(ValueError, match='ws_cap'):
            f(x, ws_cap=bad)
    with pytest.raises(ValueError, match='samples'):
        f(_fake(1, (1 << 20) + 1))


def test_fft_pow2_argument_checks():
    from segan_pytorch_amd import ops
    with pytest.raises(TypeError, match='complex128'):
        ops.fft_pow2(_fake(2, 8, torch.complex64))
    with pytest.raises(TypeError, match='tensor'):
        ops.fft_pow2([1.0, 2.0])
    for shape in ((2, 6), (2, 1), (2, 2, 4)):
        with pytest.raises(ValueError, match='fft_pow2'):
            ops.fft_pow2(torch.zeros(*shape, dtype=torch.complex128).as_subclass(_FakeCuda))
