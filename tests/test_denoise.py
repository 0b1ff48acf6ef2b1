"""Host side of the Wiener / log-MMSE baseline enhancers (the numpy oracle
scripts/denoise_oracle.py, the fixture tests/golden/denoise.pt, the header, the CLI flags, the
argument checks of ops): no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import denoise_oracle as O  # noqa: E402
import make_golden_denoise as GD  # noqa: E402


@pytest.fixture(scope='module')
def dfx():
    return load_golden('denoise.pt')


def test_exp1_against_scipy_from_2_to_minus_40_up_to_40():
    """The series adds at most 18 terms below 1 with three roundings each, and the continued
    fraction multiplies at most 92 factors (x = 1) of about three roundings each into h before
    the product with exp(-x): 300 roundings of 2^-53 bound either, scipy's own last bits
    included."""
    from scipy.special import exp1
    x = np.concatenate([2.0 ** np.linspace(-40, 0, 4001)[:-1], np.linspace(1, 40, 4001),
                        [2.0 ** -40, 1.0 - 2.0 ** -53, 1.0, 40.0]])
    got, want = O.exp1(x), exp1(x)
    rel = np.abs(got / want - 1.0)
    print('E1: worst relative distance from scipy {:.3g} (below 1: {:.3g})'.format(
        rel.max(), rel[x < 1].max()))
    assert rel.max() <= 300 * 2.0 ** -53
    ld = O.exp1(x[::50], np.longdouble)
    assert ld.dtype == np.longdouble
    assert np.abs((ld / want[::50]).astype(np.float64) - 1.0).max() <= 300 * 2.0 ** -53


def test_window_overlap_sum_is_flat():
    w = O.window(320)
    s = w[:160] + w[160:]
    assert 0.998 <= s.min() and s.max() <= 1.003, (s.min(), s.max())
    assert abs(np.sum(w) - 160.0) < 1e-12 and w[0] == w.min()
    # at 8 kHz the 160-sample window overlaps to [0.9968, 1.0053]: the same window, coarser
    w8 = O.window(160)
    s8 = w8[:80] + w8[80:]
    assert 0.996 <= s8.min() and s8.max() <= 1.006
    assert O.window(320, np.longdouble).dtype == np.longdouble


def test_constants_and_frame_counts():
    assert O.constants(16000) == (320, 160, 640) and O.constants(8000) == (160, 80, 320)
    for bad in (44100, 0, True, None):
        with pytest.raises(ValueError):
            O.constants(bad)
    assert [O.n_frames(L) for L in (1919, 1920, 2079, 2080)] == [0, 11, 11, 12]
    assert [O.n_frames(L, 8000) for L in (959, 960, 8000)] == [0, 11, 99]
    assert GD.LENGTHS == (1919, 1920, 2079, 2080, 8000, 32000)


def test_short_row_passes_through_bit_equal(dfx):
    x = dfx['signals']['noisy'].numpy()[:1919]
    for rule in O.RULES:
        r = O.denoise(x, 16000, rule)
        assert r['nframes'] == 0 and len(r['vad']) == 0 and len(r['update']) == 0
        assert r['y'].dtype == np.float64 and np.array_equal(r['y'], x.astype(np.float64))
    with pytest.raises(ValueError):
        O.denoise(x, 16000, 'mmse')


def test_zero_row_and_a_silent_start_give_no_nan(dfx):
    for rule in O.RULES:
        r = O.denoise(np.zeros(8000, np.float32), 16000, rule)
        assert r['nframes'] == 49 and not r['y'].any() and np.isfinite(r['vad']).all()
        x, _ = GD.case_rows(dfx['signals'])['silent_start']
        assert not x[:3000].any() and x[3000:].any()
        r = O.denoise(x, 16000, rule)
        assert np.isfinite(r['y']).all() and np.isfinite(r['vad']).all()
        assert not r['y'][:2720].any() and np.abs(r['y'][3200:]).max() > 0.01
        # output past (nf + 1) H is zero
        r = O.denoise(dfx['signals']['noisy'].numpy()[:2079], 16000, rule)
        assert r['y'][1920:].tolist() == [0.0] * 159 and r['y'][1800:1920].any()


@pytest.mark.parametrize('snr_db', [0, 5, 10, 20])
def test_snr_over_the_active_part_rises_by_3_db(snr_db):
    clean, active = GD.gated(GD.N, 16000)
    x = GD.add_noise(clean, active, snr_db, np.random.default_rng(100 + snr_db)).astype(np.float32)
    before = GD.active_snr(clean, x, active)
    assert abs(before - snr_db) < 0.01
    for rule in O.RULES:
        after = GD.active_snr(clean, O.denoise(x, 16000, rule)['y'], active)
        print('{:7s} {:2d} dB -> {:.2f} dB'.format(rule, snr_db, after))
        assert after >= before + 3.0, (rule, snr_db, before, after)


def test_stationary_noise_is_attenuated_by_10_db():
    for srate, n in ((16000, 16000), (8000, 8000)):
        x = (0.1 * np.random.default_rng(3).standard_normal(n)).astype(np.float32)
        F, H, _ = O.constants(srate)
        for rule in O.RULES:
            r = O.denoise(x, srate, rule)
            a, b = 6 * F, r['nframes'] * H
            att = 10 * np.log10(np.mean(x[a:b].astype(np.float64) ** 2) / np.mean(r['y'][a:b] ** 2))
            print('{:7s} {} Hz: white noise attenuated by {:.1f} dB'.format(rule, srate, att))
            assert att >= 10.0, (rule, srate, att)


def test_unit_gain_gives_the_signal_back():
    """analysis and synthesis alone: with G = 1 the overlap-add is x times the window's overlap sum"""
    F, H, N = O.constants(16000)
    x = np.random.default_rng(5).standard_normal(4 * F)
    w = O.window(F)
    C, S, Ci, Si = O.dft_tables(F)
    y = np.zeros_like(x)
    for t in range(len(x) // H - 1):
        seg = w * x[t * H:t * H + F]
        y[t * H:t * H + F] += (Ci @ (C @ seg) - Si @ (-(S @ seg))) / N
    mid = slice(H, len(x) - H)
    assert np.abs(y[mid] / x[mid] - 1.0).max() < 0.003


def test_vad_sum_grouping_is_the_documented_one():
    rng = np.random.default_rng(9)
    for F in (320, 160):
        l = rng.standard_normal(F + 1) * 10.0 ** rng.uniform(-3, 3, F + 1)
        t = 2 * l
        t[0], t[F] = l[0], l[F]
        groups = []
        for g in range(0, F + 1, 64):
            acc = 0.0
            for v in t[g:g + 64]:
                acc = acc + v
            groups.append(acc)
        want = 0.0
        for acc in groups:
            want = want + acc
        assert O.vad_sum(l, F) == want / F
        assert abs(float(O.vad_sum(l.astype(np.longdouble), F, np.longdouble)) - want / F) < 1e-9


def test_fixture_margins_tolerances_and_size(dfx):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'denoise.pt'))
    assert size < 1024 * 1024, size
    meta = dfx['meta']
    assert meta['margin_floor'] == 1e-7 and meta['min_margin'] >= 1e-7
    assert dfx['lengths'] == list(GD.LENGTHS)
    assert set(dfx['cases']) == set(GD.case_rows(dfx['signals']))
    smallest = np.inf
    for name, c in dfx['cases'].items():
        for rule in O.RULES:
            e = c[rule]
            assert len(e['vad']) == len(e['update']) == len(e['margin']) == e['nframes']
            if e['nframes']:
                m = e['margin'].numpy()
                assert np.array_equal(m, np.abs(e['vad'].numpy() - 0.15)) and m.min() >= 1e-7
                assert np.array_equal(e['update'].numpy(), e['vad'].numpy() < 0.15)
                smallest = min(smallest, m.min())
            assert ('y' in e) == (name in ('L1919', 'L1920', 'L2079', 'L2080'))
    assert smallest == meta['min_margin']
    for rule in O.RULES:
        for k in ('y', 'vad'):
            g = meta['gaps'][rule][k]
            assert 0 < g and 100 * g <= 1e-10, (rule, k, g)
            # the rounding of v_t that the margin has to cover: orders of magnitude below it
            assert 100 * g * 1e3 < meta['min_margin']
    assert [dfx['cases']['L{}'.format(L)]['wiener']['nframes'] for L in GD.LENGTHS] == [
        0, 11, 11, 12, 49, 199]
    assert dfx['cases']['rate8']['logmmse']['nframes'] == 99
    for s in dfx['signals'].values():
        assert s.dtype == torch.float32


def test_regenerating_a_case_reproduces_the_fixture(dfx):
    """The matrix products go through the BLAS of the machine, whose summation order is its own:
    v_t and y are held to the fixture's own float64-to-longdouble movement times 100, the
    decisions exactly."""
    rows = GD.case_rows(dfx['signals'])
    sig = GD.make_signals(dfx['meta']['seed'])
    for k, v in dfx['signals'].items():
        assert np.array_equal(sig[k], v.numpy()), k
    for name in ('L1919', 'L1920', 'L2080', 'L8000', 'rate8'):
        x, srate = rows[name]
        for rule in O.RULES:
            want, tol = dfx['cases'][name][rule], dfx['meta']['gaps'][rule]
            r = O.denoise(x, srate, rule)
            assert r['nframes'] == want['nframes']
            assert np.array_equal(r['update'], want['update'].numpy())
            if r['nframes']:
                dv = np.abs(r['vad'] - want['vad'].numpy()) / np.maximum(1, np.abs(r['vad']))
                assert dv.max() <= 100 * tol['vad']
            if 'y' in want:
                dy = np.abs(r['y'] - want['y'].numpy()).max() / np.abs(x).max()
                assert dy <= 100 * tol['y']
    assert np.array_equal(dfx['cases']['L1919']['wiener']['y'].numpy(),
                          rows['L1919'][0].astype(np.float64))


def test_abi_header_and_makefile_pins():
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    block = H.RAW[H.RAW.index('Wiener and log-MMSE baseline enhancers'):
                  H.RAW.index('int segan_denoise_dims')]
    assert 'Added without a change of SEGAN_ABI_VERSION: the exports\n * are purely additive.' in block
    assert H.macro('SEGAN_DENOISE_WIENER') == ops.DENOISE_RULES['wiener']
    assert H.macro('SEGAN_DENOISE_LOGMMSE') == ops.DENOISE_RULES['logmmse']
    for name, nargs in (('segan_denoise_dims', 4), ('segan_denoise', 14)):
        assert len(H.args(name)) == len(_lib.SIGNATURES[name][1]) == nargs, name
    mk = open(os.path.join(ROOT, 'Makefile')).read()
    assert '$(CSRC)/segan_denoise.hip' in mk.split('SRCS :=')[1].split('\n')[0]
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert 'segan_denoise_dims' in doc and 'segan_denoise(' in doc
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    assert lib.segan_denoise and lib.segan_denoise_dims


def test_dims_and_checks_before_any_launch():
    import ctypes
    from segan_pytorch_amd import _lib, ops
    lib = _lib.load()
    for srate in (16000, 8000):
        F = srate // 50
        for L in (1, 6 * F - 1, 6 * F, 6 * F + F // 2 - 1, 6 * F + F // 2, 8000, 32000):
            d = ops.denoise_dims(3, L, srate)
            nf = O.n_frames(L, srate)
            assert d == dict(frame=F, hop=F // 2, nfft=2 * F, frames=nf,
                             ws_bytes=3 * (16 * (F + 1) * nf + 8 * (F + 1))), (L, srate)
    one = ctypes.c_void_p(16)     # never dereferenced: the arguments are refused first
    out = (ctypes.c_int64 * 5)()

    def call(x=one, xdt=0, rows=1, T=5000, srate=16000, rule=1, y=one, ydt=2, nfr=one, ws=one):
        return lib.segan_denoise(x, xdt, None, rows, T, srate, rule, y, ydt, nfr, None, None, ws,
                                 None)

    for rows, T, srate in ((0, 5000, 16000), (65536, 5000, 16000), (1, 0, 16000),
                           (1, (1 << 24) + 1, 16000), (1, 5000, 44100), (1, 5000, 0)):
        assert lib.segan_denoise_dims(rows, T, srate, out) != 0
        assert lib.segan_last_error().startswith(b'denoise:')
        assert call(rows=rows, T=T, srate=srate) != 0
        assert b'bad sizes' in lib.segan_last_error()
    assert lib.segan_denoise_dims(1, 5000, 16000, None) != 0
    for kw in (dict(x=None), dict(y=None), dict(nfr=None), dict(ws=None)):
        assert call(**kw) != 0 and b'NULL' in lib.segan_last_error()
    for rule in (-1, 2):
        assert call(rule=rule) != 0 and b'rule' in lib.segan_last_error()
    for kw in (dict(xdt=1), dict(ydt=1), dict(xdt=3)):
        assert call(**kw) != 0 and b'SEGAN_DT_F32' in lib.segan_last_error()
    assert call(ws=ctypes.c_void_p(24)) != 0 and b'aligned' in lib.segan_last_error()


def test_clean_cli_baseline_flag():
    import clean
    p = clean.build_parser()
    base = p.parse_args([])
    assert sorted(vars(base)) == sorted(['g_pretrained_ckpt', 'test_files', 'h5', 'seed',
                                         'synthesis_path', 'cuda', 'soundfile', 'cfg_file'])
    for rule in ('wiener', 'logmmse'):
        o = p.parse_args(['--baseline', rule, '--test_files', 'd'])
        assert o.baseline == rule and o.cfg_file is None and o.g_pretrained_ckpt is None
    with pytest.raises(SystemExit):
        p.parse_args(['--baseline', 'mmse'])
    assert clean.BASELINES == ('wiener', 'logmmse')
    o = p.parse_args(['--baseline', 'wiener', '--keep_rate', '--srmr'])
    assert clean.resample_opts(o)[:2] == (True, True) and o.srmr is True
    with pytest.raises(SystemExit, match='test_files'):      # before any device is asked for
        clean.main(p.parse_args(['--baseline', 'wiener']))
    with pytest.raises(SystemExit, match='cfg_file'):
        clean.main(p.parse_args(['--test_files', 'd']))


def test_eval_cli_baseline_flag_leaves_the_header_alone():
    import eval_noisy_performance as ev
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    assert parse().baseline is None
    assert parse('--baseline', 'wiener').baseline == 'wiener'
    assert parse('--baseline', 'logmmse').baseline == 'logmmse'
    with pytest.raises(SystemExit):
        parse('--baseline', 'segan')
    for flags in ((), ('--stoi', '--sisdr'), ('--f0',)):
        assert ev.header_line(parse('--baseline', 'wiener', *flags)) == ev.header_line(parse(*flags))
    assert ev.header_line(parse('--baseline', 'wiener')) == 'FILE CSIG CBAK COVL PESQ SSNR'


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import baselines, ops
    for x in (torch.zeros(2, 5000), torch.zeros(5000, dtype=torch.float64)):
        for fn in (ops.denoise_rows, ops.denoise_stages, baselines.denoise, baselines.wiener,
                   baselines.logmmse):
            with pytest.raises(RuntimeError, match='MI355X'):
                fn(x)
    assert baselines.RULES == ('logmmse', 'wiener')


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['denoise_rows', 'denoise_stages'])
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
    with pytest.raises(ValueError, match='lengths'):
        f(_fake(5000, dtype=torch.float64), lengths=[5000, 5000])
    for bad in (0, 44100, 16000.5, True, None):
        with pytest.raises(ValueError, match='srate'):
            f(x, srate=bad)
    for bad in ('mmse', 'Wiener', 0, None, True):
        with pytest.raises(ValueError, match='rule'):
            f(x, rule=bad)
    for bad in (torch.float16, torch.int16, 'float32', 0):
        with pytest.raises(ValueError, match='out_dtype'):
            f(x, out_dtype=bad)
    for bad in (0, -1, 1.5, True, 1000):
        with pytest.raises(ValueError, match='ws_cap'):
            f(x, ws_cap=bad)
