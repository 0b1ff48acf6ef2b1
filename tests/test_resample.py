"""Host side of the sample-rate conversion (segan_resample_plan, the numpy oracle, the fixture, the
CLI flags, the declared surface): no GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
sys.path.insert(0, ROOT)
import make_golden_resample as G  # noqa: E402
import resample_oracle as R  # noqa: E402

CASES = G.cases()
NAMES = ('segan_resample_plan', 'segan_resample_dims', 'segan_resample')


@pytest.fixture(scope='module')
def rfx():
    return load_golden('resample.pt')


def _id(case):
    return '{}to{}-z{}'.format(*case[:3])


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_plan_taps_match_scipy_firwin(case):
    """segan_resample_plan's taps against scipy.signal.firwin(2 lh + 1, 1 / mx, window=('kaiser',
    beta)) p, absolute 1e-15, for every ratio and filter of the fixture.

    firwin normalises by a pairwise sum of h.  The library has one designer with two
    normalisation modes.  This, the public one, sums h in index order wherever that order's own
    rounding moves no tap by more than 1e-15 and takes a compensated sum otherwise: in index order
    the 8821 to 204801 terms of 44100 <-> 16000 and 16000 -> 12345 Hz leave the sum up to 1.1e-14
    (relative) off, and the taps with it.  STOI's mode keeps the index-order sum at every rate,
    because its taps are pinned to its oracle's bits, not to firwin."""
    from scipy.signal import firwin
    from segan_pytorch_amd import ops
    a, b, zeros, beta = case
    p, q, taps = ops.resample_plan(a, b, zeros, beta)
    mx = max(p, q)
    lh = zeros * mx
    want = firwin(2 * lh + 1, 1.0 / mx, window=('kaiser', beta)) * p
    assert taps.dtype == torch.float64 and taps.shape == (2 * lh + 1,)
    err = float(np.abs(taps.numpy() - want).max())
    print(case, 'max |taps - firwin * p| = {:.3e}'.format(err))
    assert err <= 1e-15


@pytest.mark.parametrize('srate', [4000, 8000, 16000, 22050, 44100, 48000])
def test_plan_towards_10k_with_scipys_filter_is_stois_bit_for_bit(srate):
    from segan_pytorch_amd import ops
    p, q, taps = ops.resample_plan(srate, 10000, 10, 5.0)
    sp, sq, staps, _ = ops.stoi_plan(srate)
    assert (p, q) == (sp, sq)
    assert taps.shape == staps.shape and torch.equal(taps, staps)


def test_plan_never_trades_accuracy_for_stois_bits():
    """Whatever the rate towards 10 kHz, the taps are STOI's bits or, where STOI's index-order sum
    of h is itself more than 1e-15 (in the largest tap) off the exact normalisation, within 1e-15
    of firwin; they never leave STOI's by more than the rounding of a sequential fp64 sum of n
    terms allows, (n - 1) 2^-53 relative."""
    from scipy.signal import firwin
    from segan_pytorch_amd import ops
    same = 0
    for srate in (4000, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 37800, 44100, 48000):
        p, q, taps = ops.resample_plan(srate, 10000, 10, 5.0)
        staps = ops.stoi_plan(srate)[2]
        n, peak = taps.numel(), taps.max().item()
        if torch.equal(taps, staps):
            same += 1
        else:
            want = firwin(n, 1.0 / max(p, q), window=('kaiser', 5.0)) * p
            assert np.abs(taps.numpy() - want).max() <= 1e-15, srate
        assert (taps - staps).abs().max().item() <= (n - 1) * 2.0 ** -53 * peak, srate
    assert same >= 6


def test_plan_ratio_and_tap_count():
    from segan_pytorch_amd import ops
    for (a, b, zeros), (p, q) in {(48000, 16000, 32): (1, 3), (44100, 16000, 32): (160, 441),
                                  (8000, 16000, 10): (2, 1), (16000, 44100, 10): (441, 160),
                                  (16000, 12345, 1): (2469, 3200), (192000, 4000, 64): (1, 48),
                                  (4000, 192000, 64): (48, 1)}.items():
        gp, gq, taps = ops.resample_plan(a, b, zeros, 8.6)
        assert (gp, gq) == (p, q) == R.ratio(a, b)
        assert taps.numel() == 2 * zeros * max(p, q) + 1
        assert torch.equal(taps, taps.flip(0))                     # symmetric
        assert abs(float(taps.sum()) - p) <= 1e-12 * p             # gain p at DC
    assert ops.RESAMPLE_ZEROS == 32 and ops.RESAMPLE_BETA == 8.6
    assert torch.equal(ops.resample_plan(48000, 16000)[2], ops.resample_plan(48000, 16000, 32, 8.6)[2])


def test_plan_of_equal_rates_is_the_identity():
    from segan_pytorch_amd import ops
    for rate in (4000, 16000, 192000):
        p, q, taps = ops.resample_plan(rate, rate, 7, 3.0)
        assert (p, q) == (1, 1) and taps.tolist() == [1.0]
    assert ops.resample_dims(1234, 16000, 16000)[0] == 1234


def test_dims_give_the_output_length_and_the_tile(rfx):
    from segan_pytorch_amd import ops
    for (a, b, _, _), e in rfx['cases'].items():
        for L, Ly in zip(e['lens'], e['out_lens']):
            assert ops.resample_dims(L, a, b) == (Ly, rfx['tile'])
    assert ops.resample_dims(2 ** 30, 16000, 16000)[0] == 2 ** 30


def _call_plan(lib, *args):
    pq, n = (ctypes.c_int * 2)(), ctypes.c_int()
    rc = lib.segan_resample_plan(*args, pq, ctypes.byref(n), None, 0)
    return rc, (lib.segan_last_error() or b'').decode()


def test_limits_are_reported_before_any_launch():
    """-1 for arguments that are no rates / counts / finite non-negative beta at all, -3 for
    values outside the supported limits; each with a message.  No device is touched."""
    from segan_pytorch_amd import _lib
    lib = _lib.load()
    for args, rc_want, word in [((0, 16000, 32, 8.6), -1, 'rates'), ((16000, -5, 32, 8.6), -1, 'rates'),
                                ((48000, 16000, 0, 8.6), -1, 'zeros'),
                                ((48000, 16000, 32, -1.0), -1, 'beta'),
                                ((48000, 16000, 32, float('nan')), -1, 'beta'),
                                ((48000, 16000, 32, float('inf')), -1, 'beta'),
                                ((3999, 16000, 32, 8.6), -3, '4000'),
                                ((16000, 192001, 32, 8.6), -3, '192000'),
                                ((48000, 16000, 65, 8.6), -3, 'zeros'),
                                ((48000, 16000, 32, 20.5), -3, 'beta'),
                                ((16000, 12347, 32, 8.6), -3, '4096'),
                                ((4099, 4000, 32, 8.6), -3, '4096')]:
        rc, msg = _call_plan(lib, *args)
        assert rc == rc_want and 'resample_plan' in msg and word in msg, (args, rc, msg)
    for ok in [(4000, 192000, 64, 20.0), (4096, 4095, 1, 0.0), (192000, 4000, 1, 0.0)]:
        assert _call_plan(lib, *ok)[0] == 0, ok
    pq, n, taps = (ctypes.c_int * 2)(), ctypes.c_int(), (ctypes.c_double * 8)()
    assert lib.segan_resample_plan(48000, 16000, 32, 8.6, pq, ctypes.byref(n), taps, 8) == -1
    assert b'do not fit' in lib.segan_last_error() and n.value == 193
    assert lib.segan_resample_plan(48000, 16000, 32, 8.6, None, None, None, 0) == -1
    dims = (ctypes.c_int * 2)()
    assert lib.segan_resample_dims(-1, 48000, 16000, dims) == -1
    assert lib.segan_resample_dims(2 ** 30 + 1, 16000, 16000, dims) == -3
    assert lib.segan_resample_dims(2 ** 30, 16000, 48000, dims) == -3
    assert b'2^30' in lib.segan_last_error()
    assert lib.segan_resample_dims(100, 16000, 12347, dims) == -3
    # segan_resample validates everything before it looks at a device or a pointer's contents
    one = ctypes.c_void_p(8)
    base = dict(x=one, xd=0, lens=None, rows=1, T=100, a=48000, b=16000, z=32, beta=8.6, y=one,
                yd=2, Ly=34, ol=None, nc=None, ws=None)
    for change, rc_want, word in [(dict(x=None), -1, 'NULL'), (dict(y=None), -1, 'NULL'),
                                  (dict(rows=0), -1, 'rows'), (dict(rows=65536), -1, 'rows'),
                                  (dict(T=0), -1, 'T='), (dict(xd=2), -1, 'x_dtype'),
                                  (dict(yd=3), -1, 'y_dtype'), (dict(Ly=33), -1, 'Ly_max'),
                                  (dict(yd=1, nc=one), -1, 'workspace'),
                                  (dict(a=3000), -3, '4000'), (dict(z=100), -3, 'zeros'),
                                  (dict(beta=21.0), -3, 'beta'), (dict(b=16001), -3, '4096'),
                                  (dict(a=4000, b=192000, T=2 ** 25), -3, '2^30')]:
        k = dict(base, **change)
        rc = lib.segan_resample(k['x'], k['xd'], k['lens'], k['rows'], k['T'], k['a'], k['b'], k['z'],
                                k['beta'], k['y'], k['yd'], k['Ly'], k['ol'], k['nc'], k['ws'], None)
        msg = (lib.segan_last_error() or b'').decode()
        assert rc == rc_want and msg.startswith('resample:') and word in msg, (change, rc, msg)


def test_ops_reject_bad_arguments_with_a_clear_error():
    from segan_pytorch_amd import ops
    for bad in [(3999, 16000), (16000, 192001), (16000.0, 16000), ('48000', 16000), (None, 16000),
                (True, 16000)]:
        with pytest.raises(ValueError, match='rate'):
            ops.resample_plan(*bad)
    for zeros, beta in [(0, 8.6), (65, 8.6), (2.5, 8.6), (32, -0.1), (32, 20.1), (32, 'x'),
                        (32, float('nan'))]:
        with pytest.raises(ValueError, match='zeros|beta'):
            ops.resample_plan(48000, 16000, zeros, beta)
    with pytest.raises(RuntimeError, match='4096'):
        ops.resample_plan(16000, 12347)
    x = torch.zeros(2, 300)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.resample(x, 48000, 16000)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.resample(x.to(torch.int16), 48000, 16000)
    with pytest.raises(TypeError, match='tensor'):
        ops.resample(x.numpy(), 48000, 16000)


def test_ops_reject_wrong_dtypes_and_shapes():
    """The dtype, shape and rate checks of ops.resample come before it needs a device; a meta
    tensor stands in for a CUDA one."""
    from segan_pytorch_amd import ops
    if not torch.cuda.is_available():
        class Fake(torch.Tensor):
            is_cuda = True
        def fake(t):
            return t.as_subclass(Fake)
    else:
        def fake(t):
            return t.cuda()
    for dt in (torch.float64, torch.int32, torch.float16, torch.uint8):
        with pytest.raises(TypeError, match='float32 or int16'):
            ops.resample(fake(torch.zeros(2, 300, dtype=dt)), 48000, 16000)
    x = fake(torch.zeros(2, 300))
    with pytest.raises(TypeError, match='out_dtype'):
        ops.resample(x, 48000, 16000, out_dtype=torch.int32)
    with pytest.raises(ValueError, match=r'\[rows, T\]'):
        ops.resample(fake(torch.zeros(300)), 48000, 16000)
    with pytest.raises(ValueError, match=r'\[rows, T\]'):
        ops.resample(fake(torch.zeros(0, 300)), 48000, 16000)
    with pytest.raises(ValueError, match='contiguous'):
        ops.resample(fake(torch.zeros(300, 2).t()), 48000, 16000)
    with pytest.raises(ValueError, match='rate'):
        ops.resample(x, 48000, 1000)
    with pytest.raises(ValueError, match='lengths'):
        ops.resample(x, 48000, 16000, lengths=[1, 2, 3])
    with pytest.raises(ValueError, match='lengths'):
        ops.resample(x, 48000, 16000, lengths=[1, 301])


@pytest.mark.parametrize('rates', G.RATES, ids=lambda r: '{}to{}'.format(*r))
def test_oracle_equals_scipy_resample_poly(rates):
    rng = np.random.default_rng(11)
    for zeros, beta in G.FILTERS:
        p, q, taps = R.plan(rates[0], rates[1], zeros, beta)
        for L in (1, 2, 7, 257, 700):
            x = rng.standard_normal(L)
            y, ys = R.resample(x, p, q, taps), R.resample_scipy(x, p, q, taps)
            assert y.shape == ys.shape == (R.out_len(L, p, q),)
            assert np.abs(y - ys).max() <= 1e-12 * np.abs(y).max(), (rates, zeros, L)
    # scipy's own default filter is (10, 5.0)
    from scipy.signal import resample_poly
    p, q, taps = R.plan(rates[0], rates[1], R.SCIPY_ZEROS, R.SCIPY_BETA)
    x = rng.standard_normal(300)
    y = R.resample(x, p, q, taps)
    assert np.abs(y - resample_poly(x, p, q)).max() <= 1e-12 * np.abs(y).max()


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_oracle_reproduces_the_fixture(rfx, case):
    e = rfx['cases'][case]
    got = G.expected_for(case, e['seed'])
    assert got['lens'] == e['lens'] == G.row_lengths(*case[:3]) and got['out_lens'] == e['out_lens']
    assert sum(e['out_lens']) == e['y64'].numel() == e['y16'].numel()
    peak = e['y64'].abs().max().item()
    assert np.abs(got['y64'] - e['y64'].numpy()).max() <= 1e-13 * peak
    assert np.array_equal(got['y16'], e['y16'].numpy())
    assert np.array_equal(got['sq16'], e['sq16'].numpy()) and got['sq_nclip'] == e['sq_nclip'] > 0
    assert e['margin'] >= G.HALF_MARGIN and got['margin'] >= G.HALF_MARGIN
    sat = (e['sq16'] == 32767) | (e['sq16'] == -32768)
    assert e['sq_peak'] > 36000 and int(sat.sum()) >= e['sq_nclip']


def test_fixture_rows_cover_the_tile_edges(rfx):
    assert rfx['tile'] == G.TILE and set(rfx['cases']) == set(CASES)
    tile = rfx['tile']
    for case, e in rfx['cases'].items():
        lens, outs = e['lens'], e['out_lens']
        assert lens[:3] == [0, 1, 2]
        p, q = e['p'], e['q']
        assert 2 < lens[3] < 2 * case[2] * max(p, q) // p + 1          # shorter than the filter
        assert min(o for o in outs if o >= tile - 1) <= tile + 1
        assert any(o > tile for o in outs)
        if case[:2] == (16000, 12345):
            assert max(lens) == 700 and p == 2469
        else:
            assert max(outs) > 3 * tile
    # size: well under stoi.pt
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'resample.pt'))
    assert size < os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'stoi.pt')) // 2


def test_to_int16_rounds_half_to_even_and_saturates():
    y, n = R.to_int16([0.5, 1.5, 2.5, -0.5, -1.5, 32767.4, 32767.5, 40000.0, -32768.5, -32769.0, -1e9])
    assert y.tolist() == [0, 2, 2, 0, -2, 32767, 32767, 32767, -32768, -32768, -32768]
    assert n == 4


def test_new_flags_parse():
    import clean
    import eval_noisy_performance as ev
    import make_pcm_shard
    import train
    parse = clean.build_parser().parse_args
    assert clean.resample_opts(parse([])) == (False, False, 32, 8.6)
    assert clean.resample_opts(parse(['--resample'])) == (True, False, 32, 8.6)
    assert clean.resample_opts(parse(['--keep_rate'])) == (True, True, 32, 8.6)       # implies --resample
    assert clean.resample_opts(parse(['--resample', '--keep_rate', '--resample_zeros', '10',
                                      '--resample_beta', '5.0'])) == (True, True, 10, 5.0)
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    d = ev.build_parser().parse_args(req)
    assert (d.resample, d.resample_zeros, d.resample_beta, d.stoi) == (False, 32, 8.6, False)
    o = ev.build_parser().parse_args(req + ['--resample', '--resample_zeros', '16'])
    assert o.resample is True and o.resample_zeros == 16
    d = make_pcm_shard.build_parser().parse_args(['c', 'n', 'out'])
    assert (d.resample, d.resample_zeros, d.resample_beta, d.slice_size) == (False, 32, 8.6, 16384)
    o = make_pcm_shard.build_parser().parse_args(['c', 'n', 'out', '--resample', '--resample_beta', '6'])
    assert o.resample is True and o.resample_beta == 6.0
    assert train.build_parser().parse_args([]).additive_resample is False
    o = train.build_parser().parse_args(['--pcm_shard', 'sh', '--additive_noises', 'd',
                                         '--additive_resample'])
    assert o.additive_resample is True and train.check_additive_flags(o) is True


def test_additive_resample_needs_additive_noises():
    import train
    for argv in (['--additive_resample'], ['--pcm_shard', 'sh', '--additive_resample']):
        with pytest.raises(SystemExit, match='--additive_resample needs --additive_noises'):
            train.check_additive_flags(train.build_parser().parse_args(argv))
    with pytest.raises(SystemExit, match='only together with --pcm_shard'):
        train.check_additive_flags(train.build_parser().parse_args(
            ['--additive_noises', 'd', '--additive_resample']))


def test_header_signatures_and_integration_notes_agree():
    from segan_pytorch_amd import _lib
    notes = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(H.args(name)), name
        assert '`{}`'.format(name) in notes, name
    assert [n for n in _lib.SIGNATURES if 'resample' in n] == list(NAMES)
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    from segan_pytorch_amd import ops
    for macro, dt in (('SEGAN_DT_F32', torch.float32), ('SEGAN_DT_I16', torch.int16),
                      ('SEGAN_DT_F64', torch.float64)):
        assert H.macro(macro) == ops._RESAMPLE_DT[dt]


def test_host_helpers_need_no_device_at_the_target_rate(tmp_path):
    """Arrays already at the target rate come back as the same objects, and a shard built with
    target_rate from 16 kHz files holds the bytes of one built without it."""
    from scipy.io import wavfile
    from segan_pytorch_amd import resample
    from segan_pytorch_amd.augment import NoiseBank
    from segan_pytorch_amd.datasets import build_pcm_shard
    a = np.arange(10, dtype=np.int16)
    b = np.ones((5, 2), dtype=np.float64)
    out, nclip = resample.resample_many([a, b], [16000, 16000])
    assert out[0] is a and out[1] is b and nclip == 0
    assert resample.resample_wav(a, 16000) is a
    assert resample.resample_many([], 48000) == ([], 0)
    with pytest.raises(ValueError, match='rates'):
        resample.resample_many([a], [16000, 16000])
    stereo = np.array([[1, 2], [3, 4], [-5, 6]], dtype=np.int16)
    assert resample.as_mono(stereo).dtype == np.float32
    assert resample.as_mono(stereo).tolist() == [1.5, 3.5, 0.5]
    assert resample.as_mono(a).dtype == np.int16 and resample.as_mono(b).dtype == np.float32
    with pytest.raises(TypeError, match='int16 or float'):
        resample.as_mono(np.zeros(4, dtype=np.int32))
    rng = np.random.default_rng(3)
    cd, nd = tmp_path / 'clean', tmp_path / 'noisy'
    cd.mkdir()
    nd.mkdir()
    for i in range(2):
        c = (rng.standard_normal(3000) * 4000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000, (c // 2).astype(np.int16))
    n0 = build_pcm_shard(str(cd), str(nd), str(tmp_path / 'a'), slice_size=1024)
    n1 = build_pcm_shard(str(cd), str(nd), str(tmp_path / 'b'), slice_size=1024, target_rate=16000)
    assert n0 == n1 > 0
    assert (tmp_path / 'a.pcm16').read_bytes() == (tmp_path / 'b.pcm16').read_bytes()
    assert (tmp_path / 'a.json').read_bytes() == (tmp_path / 'b.json').read_bytes()
    bank = NoiseBank.from_dir(str(cd), target_rate=16000)
    assert np.array_equal(bank.host, NoiseBank.from_dir(str(cd)).host)
