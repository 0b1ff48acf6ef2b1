"""Host side of the WPE dereverberation baseline (the numpy oracle scripts/wpe_oracle.py, the
fixture tests/golden/wpe.pt, the extension header include/segan_dereverb.h, the CLI flags, the
argument checks of the library and of ops): no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import wpe_oracle as O  # noqa: E402
import make_golden_wpe as GW  # noqa: E402


@pytest.fixture(scope='module')
def wfx():
    return load_golden('wpe.pt')


@pytest.fixture(scope='module')
def rows(wfx):
    return GW.case_rows({k: v.numpy() for k, v in wfx['signals'].items()})


def test_constants_frame_counts_and_parameter_ranges():
    assert O.constants(16000) == (512, 128, 257) and O.constants(8000) == (256, 64, 129)
    for bad in (44100, 0, True, None):
        with pytest.raises(ValueError):
            O.constants(bad)
    assert [O.n_frames(L) for L in (0, 1, 127, 128, 129, 1280, 1281, 8000, 32000)] == [
        3, 4, 4, 4, 5, 13, 14, 66, 253]
    assert [O.n_frames(L, 8000) for L in GW.tile_lengths()] == [511, 512, 513]
    x = np.zeros(4000, np.float32)
    for kw in (dict(taps=0), dict(taps=33), dict(delay=0), dict(delay=9), dict(iterations=-1),
               dict(iterations=9), dict(taps=2.0), dict(delay=True)):
        with pytest.raises(ValueError):
            O.wpe(x, **kw)


def test_window_squares_overlap_to_two_and_the_fft_is_numpys():
    for N in (512, 256):
        w = O.window(N)
        s = sum(w[q * N // 4:(q + 1) * N // 4] ** 2 for q in range(4))
        assert np.abs(s - 2.0).max() < 1e-14
        assert O.window(N, np.longdouble).dtype == np.longdouble
    z = np.random.RandomState(2).standard_normal((3, 512)) + 1j * np.random.RandomState(3).standard_normal((3, 512))
    assert np.abs(O.fft(z) - np.fft.fft(z)).max() < 1e-12
    assert np.abs(O.fft(z, inverse=True) / 512 - np.fft.ifft(z)).max() < 1e-14
    assert O.fft(z[:, :256], dtype=np.longdouble).dtype == np.clongdouble


def test_solve_is_a_cholesky_solve():
    rng = np.random.RandomState(4)
    A = rng.standard_normal((5, 7, 12)) + 1j * rng.standard_normal((5, 7, 12))
    R = A @ np.conj(np.swapaxes(A, 1, 2))
    P = rng.standard_normal((5, 7)) + 1j * rng.standard_normal((5, 7))
    g, ok = O.solve(R, P)
    assert ok.all() and np.abs(g - np.linalg.solve(R, P[..., None])[..., 0]).max() < 1e-12
    R[2] = -R[2]                                   # not positive definite: g = 0, flagged
    g, ok = O.solve(R, P)
    assert ok.tolist() == [True, True, False, True, True] and not g[2].any() and g[1].any()
    gl, _ = O.solve(R.astype(np.clongdouble), P.astype(np.clongdouble), np.longdouble)
    assert gl.dtype == np.clongdouble


def test_oracle_reproduces_the_fixture(wfx, rows):
    """Against the fixture's subsample, to 100 times the fixture's own float64-to-longdouble
    movement of the case: numpy's pairwise sums may group differently on another machine."""
    assert set(wfx['cases']) == set(rows)
    for name in ('L1', 'L1280', 'L1281', 'L8000', 'rate8', 'zero', 'scaled', 'band4k', 'taps1',
                 'delay8', 'iterations0', 'iterations1'):
        x, srate, kw = rows[name]
        want = wfx['cases'][name]
        assert {k: want[k] for k in kw} == kw and want['srate'] == srate
        r = O.wpe(x, srate, **kw)
        assert r['nframes'] == want['nframes'] and r['status'] == want['status'] == 0
        sub = GW.subsample(r)
        peak, ypeak = float(np.abs(x).max()), float(np.abs(r['Y']).max())
        for k, scale in (('y', peak), ('X', ypeak), ('g', 1.0)):
            d = float(np.abs(sub[k] - want[k].numpy()).max()) if sub[k].size else 0.0
            assert d <= 100 * want['gaps'][k] * scale, (name, k, d)


def test_fixture_shape_and_size(wfx, rows):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'wpe.pt'))
    assert size < 600 * 1024, size
    assert wfx['lengths'] == list(GW.LENGTHS) == [1, 127, 128, 129, 1280, 1281, 8000, 32000]
    assert wfx['meta']['tile'] == GW.TILE
    for k, v in wfx['signals'].items():
        assert v.dtype == (torch.float32 if k == 'band4k' else torch.int16), k
    sig = GW.make_signals(wfx['meta']['seed'])
    assert set(sig) == set(wfx['signals'])
    for name, c in wfx['cases'].items():
        x, srate, kw = rows[name]
        assert c['nframes'] == O.n_frames(len(x), srate)
        short = c['nframes'] <= kw['delay'] + kw['taps']
        assert (c['gaps']['y'] == 0) == (short or name == 'zero'), name
        assert all(0 <= c['gaps'][k] < 1e-4 for k in ('y', 'X', 'g')), (name, c['gaps'])
    # the band-limited row's upper bins are nearly empty (away from the row's two ends, where the
    # frames see it cut off): the window's leakage, 88 dB down
    Y = O.stft(rows['band4k'][0])
    assert np.abs(Y[140:, 4:-4]).max() < 1e-4 * np.abs(Y).max()


def test_zero_iterations_is_the_identity_to_rounding(rows):
    for name in ('L8000', 'rate8'):
        x, srate, kw = rows[name]
        r = O.wpe(x, srate, **dict(kw, iterations=0))
        assert np.abs(r['y'] - x).max() <= 1e-14 * np.abs(x).max()
        assert np.array_equal(r['X'], r['Y']) and not r['g'].any()
    x = rows['L8000'][0]
    r = O.wpe(x, iterations=0, dtype=np.longdouble)
    assert r['y'].dtype == np.longdouble and float(np.abs(r['y'] - x).max()) < 1e-17


def test_a_power_of_two_scales_every_bit(rows):
    x, _, kw = rows['L8000']
    a = O.wpe(x, **kw)
    for e in (-10, 7):
        b = O.wpe(x * np.float32(2.0 ** e), **kw)
        assert np.array_equal(b['y'] * 2.0 ** -e, a['y'])
        assert np.array_equal(b['X'] * 2.0 ** -e, a['X']) and np.array_equal(b['g'], a['g'])
    assert np.array_equal(rows['scaled'][0] * np.float32(1024), x)


def test_short_rows_come_back_unchanged(rows):
    """nf = delay + taps is the last row left alone, nf = delay + taps + 1 the first one
    filtered."""
    x = rows['L1281'][0]
    for L, nf in ((1, 4), (128, 4), (1280, 13)):
        r = O.wpe(x[:L])
        assert r['nframes'] == nf and r['y'].dtype == np.float64
        assert np.array_equal(r['y'], x[:L].astype(np.float64))
        assert np.array_equal(r['X'], r['Y']) and not r['g'].any() and r['g'].shape == (257, 10)
    r = O.wpe(x)
    assert r['nframes'] == 14 and r['g'].any() and not np.array_equal(r['y'], x.astype(np.float64))
    assert O.wpe(x[:1280], taps=9)['g'].any()          # 13 frames > 3 + 9
    assert not O.wpe(x, delay=4)['g'].any()            # 14 frames = 4 + 10
    e = O.wpe(np.zeros(0, np.float32))
    assert e['nframes'] == 3 and e['y'].shape == (0,)


def test_zero_row_and_silent_start_give_no_nan(rows):
    r = O.wpe(np.zeros(8000, np.float32))
    assert r['nframes'] == 66 and r['status'] == 0
    assert not r['y'].any() and not r['g'].any() and not r['X'].any()
    x = rows['silent_start'][0]
    assert not x[:3000].any() and x[3000:].any()
    r = O.wpe(x)
    assert np.isfinite(r['y']).all() and np.isfinite(r['g'].view(np.float64)).all()
    assert r['status'] == 0 and np.abs(r['y'][:2500]).max() < 1e-12 * np.abs(x).max()


def test_wpe_lowers_the_residual_against_the_early_target(wfx):
    """The physical property, on the oracle: the energy of (signal - early-reflection target) falls.
    Measured when the fixture was made: 1.46 dB (RT60 0.3 s, 1 s) and 1.58 dB (RT60 0.6 s, 2 s)
    with 10 taps, a delay of 3 and 3 iterations; half of the measured value is asserted, which
    leaves room for a deliberate change of the defaults."""
    sig = {k: v.numpy() for k, v in wfx['signals'].items()}
    meta = wfx['meta']['improvement_db']
    assert abs(meta['03'] - 1.46) < 0.01 and abs(meta['06'] - 1.58) < 0.01
    for name in ('03', '06'):
        got = GW.improvement_db(sig, name)
        print('RT60 0.{} s: residual against the early target lowered by {:.2f} dB (fixture '
              '{:.2f})'.format(name[1], got, meta[name]))
        assert got >= 0.5 * meta[name], (name, got)
    # zero iterations change nothing
    assert abs(GW.improvement_db(sig, '03', iterations=0)) < 1e-9


def test_extension_header_binding_and_makefile():
    from segan_pytorch_amd import _lib, ops
    assert len(_lib.SIGNATURES) == 119 and _lib.ABI_VERSION == 17
    assert not [n for n in _lib.SIGNATURES if n.startswith('segan_wpe')]
    assert not [n for n in _lib.DEFINES if n.startswith('SEGAN_WPE')]
    with open(_lib.EXT_HEADER_PATH) as f:
        raw = f.read()
    sig, defs = _lib.read_header(raw, 'segan_dereverb.h')
    assert list(sig) == list(_lib.EXT_SIGNATURES) == ['segan_wpe_dims', 'segan_wpe']
    assert sig == _lib.EXT_SIGNATURES and dict(defs) == dict(_lib.EXT_DEFINES)
    assert [len(_lib.EXT_SIGNATURES[n][1]) for n in ('segan_wpe_dims', 'segan_wpe')] == [6, 18]
    assert dict(defs) == {'SEGAN_WPE_MAX_TAPS': 32, 'SEGAN_WPE_MAX_DELAY': 8,
                          'SEGAN_WPE_MAX_ITERATIONS': 8, 'SEGAN_WPE_TILE': 512,
                          'SEGAN_WPE_ST_PIVOT': 2}
    assert (ops.WPE_MAX_TAPS, ops.WPE_MAX_DELAY, ops.WPE_MAX_ITERATIONS, ops.WPE_TILE,
            ops.WPE_PIVOT) == (32, 8, 8, 512, 2)
    assert (O.TAPS[1], O.DELAY[1], O.ITERATIONS[1], O.ST_PIVOT, GW.TILE) == (32, 8, 8, 2, 512)
    assert ops.WPE_WS_CAP == 1 << 30
    assert 'purely additive' in raw and 'SEGAN_ABI_VERSION stays 17' in raw
    with pytest.raises(RuntimeError, match='not found'):
        _lib._read_header_file(os.path.join(ROOT, 'include', 'no_such_header.h'))
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert '$(CSRC)/segan_dereverb.hip' in mk.split('SRCS :=')[1].split('\n')[0]
    assert 'include/segan_dereverb.h' in mk and '$(CSRC)/segan_fft_lds.h' in mk
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'segan_dereverb.h' in doc and 'segan_wpe_dims' in doc and 'segan_wpe(' in doc
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    assert lib.segan_wpe.argtypes == _lib.EXT_SIGNATURES['segan_wpe'][1]
    assert lib.segan_wpe_dims.restype is ctypes.c_int


def test_dims_and_checks_before_any_launch():
    from segan_pytorch_amd import _lib, ops
    lib = _lib.load()
    for srate in (16000, 8000):
        N, H, F = O.constants(srate)
        for L in (1, H - 1, H, H + 1, 10 * H, 8000, 32000, 1 << 24):
            d = ops.wpe_dims(3, L, srate)
            nf = O.n_frames(L, srate)
            assert d == dict(nfft=N, hop=H, bins=F, frames=nf,
                             ws_bytes=3 * (32 * F * nf + 4 * (F + 3))), (L, srate)
    assert ops.wpe_dims(1, 64000)['ws_bytes'] > 4 * 10 ** 6        # 824 such rows need chunks
    one = ctypes.c_void_p(16)     # never dereferenced: the arguments are refused first
    out = (ctypes.c_int64 * 5)()

    def call(x=one, xdt=0, rows=1, T=5000, srate=16000, taps=10, delay=3, it=3, y=one, ydt=2,
             nfr=one, status=one, Y=None, X=None, g=None, ws=one):
        return lib.segan_wpe(x, xdt, None, rows, T, srate, taps, delay, it, y, ydt, nfr, status, Y,
                             X, g, ws, None)

    for rows, T, srate in ((0, 5000, 16000), (65536, 5000, 16000), (1, 0, 16000),
                           (1, (1 << 24) + 1, 16000), (1, 5000, 44100), (1, 5000, 0)):
        assert lib.segan_wpe_dims(rows, T, srate, 10, 3, out) != 0
        assert lib.segan_last_error().startswith(b'wpe:')
        assert call(rows=rows, T=T, srate=srate) != 0
        assert lib.segan_last_error().startswith(b'wpe: bad sizes')
    assert lib.segan_wpe_dims(1, 5000, 16000, 10, 3, None) != 0
    assert lib.segan_last_error().startswith(b'wpe: NULL')
    for kw in (dict(x=None), dict(y=None), dict(nfr=None), dict(status=None), dict(ws=None)):
        assert call(**kw) != 0 and lib.segan_last_error().startswith(b'wpe: NULL')
    for taps, delay in ((0, 3), (33, 3), (-1, 3), (10, 0), (10, 9)):
        assert lib.segan_wpe_dims(1, 5000, 16000, taps, delay, out) != 0
        assert b'taps' in lib.segan_last_error()
        assert call(taps=taps, delay=delay) != 0 and b'delay' in lib.segan_last_error()
    for it in (-1, 9):
        assert call(it=it) != 0 and b'iterations' in lib.segan_last_error()
    for kw in (dict(xdt=1), dict(ydt=1), dict(xdt=3), dict(ydt=-1)):
        assert call(**kw) != 0 and b'SEGAN_DT_F32' in lib.segan_last_error()
    for kw in (dict(ws=ctypes.c_void_p(24)), dict(Y=ctypes.c_void_p(8)),
               dict(X=ctypes.c_void_p(40)), dict(g=ctypes.c_void_p(4))):
        assert call(**kw) != 0 and b'aligned' in lib.segan_last_error()
        assert lib.segan_last_error().startswith(b'wpe:')


def test_clean_cli_wpe_flags():
    import clean
    from segan_pytorch_amd.baselines import wpe_opts
    p = clean.build_parser()
    assert sorted(vars(p.parse_args([]))) == sorted([
        'g_pretrained_ckpt', 'test_files', 'h5', 'seed', 'synthesis_path', 'cuda', 'soundfile',
        'cfg_file'])
    assert clean.BASELINES == ('wiener', 'logmmse')
    with pytest.raises(SystemExit):
        p.parse_args(['--baseline', 'wpe'])
    o = p.parse_args(['--wpe', '--test_files', 'd'])
    assert o.wpe is True and o.cfg_file is None and not hasattr(o, 'baseline')
    assert wpe_opts(o) == {'taps': 10, 'delay': 3, 'iterations': 3}
    o = p.parse_args(['--wpe', '--wpe_taps', '20', '--wpe_delay', '2', '--wpe_iterations', '5',
                      '--baseline', 'wiener', '--keep_rate', '--srmr'])
    assert wpe_opts(o) == {'taps': 20, 'delay': 2, 'iterations': 5}
    assert o.baseline == 'wiener' and clean.resample_opts(o)[:2] == (True, True) and o.srmr is True
    assert wpe_opts(p.parse_args([])) is None
    with pytest.raises(SystemExit, match='needs --wpe'):
        wpe_opts(p.parse_args(['--wpe_taps', '5']))
    with pytest.raises(SystemExit, match='test_files'):      # before any device is asked for
        clean.main(p.parse_args(['--wpe']))
    with pytest.raises(SystemExit, match='--wpe does not go with --cfg_file'):
        clean.main(p.parse_args(['--wpe', '--cfg_file', 'train.opts', '--test_files', 'd']))
    with pytest.raises(SystemExit, match='cfg_file'):
        clean.main(p.parse_args(['--test_files', 'd']))


def test_eval_cli_wpe_flags_leave_the_header_alone():
    import eval_noisy_performance as ev
    from segan_pytorch_amd.baselines import wpe_opts
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    assert not hasattr(parse(), 'wpe') and wpe_opts(parse()) is None
    assert wpe_opts(parse('--wpe')) == {'taps': 10, 'delay': 3, 'iterations': 3}
    assert wpe_opts(parse('--wpe', '--wpe_taps', '30', '--wpe_iterations', '1')) == {
        'taps': 30, 'delay': 3, 'iterations': 1}
    o = parse('--wpe', '--baseline', 'logmmse')
    assert o.baseline == 'logmmse' and wpe_opts(o) is not None
    with pytest.raises(SystemExit, match='needs --wpe'):
        wpe_opts(parse('--wpe_delay', '2'))
    for flags in ((), ('--stoi', '--srmr'), ('--f0',), ('--baseline', 'wiener')):
        assert ev.header_line(parse('--wpe', *flags)) == ev.header_line(parse(*flags))
    assert ev.header_line(parse('--wpe')) == 'FILE CSIG CBAK COVL PESQ SSNR'


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import baselines, ops
    for x in (torch.zeros(2, 5000), torch.zeros(5000, dtype=torch.float64)):
        for fn in (ops.wpe_rows, ops.wpe_stages, baselines.wpe):
            with pytest.raises(RuntimeError, match='MI355X'):
                fn(x)
    with pytest.raises(TypeError, match='int16 or float'):
        baselines.wpe_wav(np.zeros((5000, 2), np.int16))
    with pytest.raises(TypeError, match='int16 or float'):
        baselines.wpe_wav(np.zeros(5000, np.int32))
    assert baselines.RULES == ('logmmse', 'wiener') and sorted(ops.DENOISE_RULES) == list(baselines.RULES)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['wpe_rows', 'wpe_stages'])
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
    for bad in (0, 33, 2.5, True, None):
        with pytest.raises(ValueError, match='taps'):
            f(x, taps=bad)
    for bad in (0, 9, 1.0, False):
        with pytest.raises(ValueError, match='delay'):
            f(x, delay=bad)
    for bad in (-1, 9, 3.0, True):
        with pytest.raises(ValueError, match='iterations'):
            f(x, iterations=bad)
    for bad in (torch.float16, torch.int16, 'float32', 0):
        with pytest.raises(ValueError, match='out_dtype'):
            f(x, out_dtype=bad)
    for bad in (0, -1, 1.5, True, 1000):
        with pytest.raises(ValueError, match='ws_cap'):
            f(x, ws_cap=bad)
