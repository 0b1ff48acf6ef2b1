"""Host side of the room-impulse-response synthesis: the physics of the numpy
oracle scripts/rir_oracle.py, the fixture tests/golden/rir.pt against its recipe, the room draws,
the nominal reverberation time, the header, the binding, the Makefile, the argument checks of the
library that need no GPU, and the flags of train.py and scripts/synth_rirs.py.

The device parity is tests/test_gpu_rir.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_rir as GR  # noqa: E402
import rir_oracle as R  # noqa: E402

ROOM, SRC, MIC = np.array(GR.ROOM), np.array(GR.SRC), np.array(GR.MIC)


@pytest.fixture(scope='module')
def rfx():
    return load_golden('rir.pt')


# ---- the oracle's physics -----------------------------------------------------------------------

@pytest.mark.parametrize('srate', [16000, 8000])
def test_dead_walls_leave_the_direct_path(srate):
    o = R.rir(ROOM, SRC, MIC, [0.0] * 6, 300, srate)
    d = float(np.linalg.norm(SRC - MIC))
    tau = d * srate / R.C
    h = o['h']
    assert abs(int(np.argmax(np.abs(h))) - tau) <= 1.0
    Hw = R.half_width(srate)
    lo, hi = int(np.floor(tau)) - Hw, int(np.floor(tau)) + Hw + 1
    assert not h[:lo].any() and not h[hi:].any()          # nothing but the one impulse
    # The taps sum to the impulse's spectrum at the multiples of the rate: the ideal low-pass
    # (1 on |v| < 1/2) convolved with the Hann window's transform W(v) = Hw sinc(x) / (1 - x^2),
    # x = 2 Hw v, whose integral is w(0) = 1.  Beyond |v| = 1/2, |W| <= 1.01 / (8 pi Hw^2 |v|^3), and
    # the integral of that over both tails is 1.01 / (2 pi Hw^2): what the term at 0 misses of 1,
    # and a bound of all the other terms together.  So the sum is within 1.01 / (pi Hw^2) of 1,
    # whatever the fraction of the delay.
    gain = h.sum() * 4.0 * np.pi * d
    print('tap sum of the direct path at {} Hz: 1 {:+.3e}, bound {:.3e}'.format(
        srate, gain - 1.0, 1.01 / (np.pi * Hw * Hw)))
    assert abs(gain - 1.0) <= 1.01 / (np.pi * Hw * Hw)
    one = R.rir(ROOM, SRC, MIC, [0.0, 0.9, 0.9, 0.9, 0.9, 0.9], 300, srate)['h']
    assert np.abs(one - h).max() > 0                      # a single dead wall is not a dead room


def test_an_image_on_a_sample_is_one_tap():
    # d = 343 / 16000 * 100 m along x: tau = 100 exactly, f = 0, the sinc is 1 at k' = 0 and 0 elsewhere
    d = 100 * R.C / 16000
    o = R.rir([10, 10, 10], [2.0, 5.0, 5.0], [2.0 + d, 5.0, 5.0], [0.0] * 6, 256)
    h = o['h']
    tau = np.sqrt((d * d + 0.0) + 0.0) * (16000 / R.C)
    if tau == 100.0:
        assert h[100] == 1.0 / ((4.0 * np.pi) * d) and np.abs(np.delete(h, 100)).max() < 1e-17
    else:      # a rounding of d moved tau off the sample: still the peak
        assert int(np.argmax(np.abs(h))) == 100


def test_source_and_receiver_swap():
    beta = [0.9, 0.7, 0.5, 0.85, 0.6, 0.95]
    a = R.rir(ROOM, SRC, MIC, beta, 1024)
    b = R.rir(ROOM, MIC, SRC, beta, 1024)
    move = float(np.abs(R.rir(ROOM, SRC, MIC, beta, 1024, dtype=np.longdouble)['h'] - a['h']).max())
    gap = float(np.abs(a['h'] - b['h']).max())
    print('reciprocity: gap {:.3e}, movement {:.3e}'.format(gap, move))
    assert a['images'] == b['images'] and move > 0
    assert gap <= 100 * move


def test_energy_rises_with_beta():
    e = [float((R.rir(ROOM, SRC, MIC, [b] * 6, 1024)['h'] ** 2).sum()) for b in (0.0, 0.3, 0.6, 0.9)]
    assert e[0] < e[1] < e[2] < e[3]


def test_t30_rises_with_the_nominal_rt60():
    from segan_pytorch_amd.augment import beta_from_rt60
    room, srate = np.array([8.0, 6.0, 3.5]), 8000
    t30 = []
    for rt60 in (0.2, 0.4, 0.6):
        beta = float(beta_from_rt60(room, rt60))
        h = R.rir(room, [2.1, 1.7, 1.3], [5.6, 4.2, 1.6], [beta] * 6, int(1.5 * rt60 * srate),
                  srate)['h']
        t30.append(R.schroeder_t30(h, srate))
        print('nominal {:.1f} s: beta {:.4f}, T30 {:.3f} s, ratio {:.2f}'.format(
            rt60, beta, t30[-1], t30[-1] / rt60))
    assert t30[0] < t30[1] < t30[2]       # the order alone: the figure is nominal


def test_the_enumeration_is_a_superset_and_the_tables_are_cumulative_products():
    from segan_pytorch_amd import ops
    beta = np.array([[0.0, 1.0, 0.5, 0.81, 0.3, 0.95], [0.9] * 6])
    tab = ops.rir_tables(beta, 7)
    assert tab.shape == (2, 6, 8) and tab.dtype == np.float64
    assert tab[0, 0].tolist() == [1.0] + [0.0] * 7 and tab[0, 1].tolist() == [1.0] * 8
    v = 1.0
    for i in range(8):
        assert tab[0, 3, i] == v
        v = v * 0.81
    assert ops.rir_tables([0.5] * 6, 0).shape == (1, 6, 1)
    # A longer row leaves the samples of the shorter one alone but for the order of the sum: n
    # images reach the short row, no tap is above the direct path's M = 1 / (4 pi d) (beta <= 1,
    # |window sinc| <= 1), and another order of n terms below M moves a sum by n^2 2^-52 M at most.
    short = R.rir(ROOM, SRC, MIC, [0.81] * 6, 400)
    a, n = short['h'], short['images']
    b = R.rir(ROOM, SRC, MIC, [0.81] * 6, 900)['h'][:400]
    M = 1.0 / (4.0 * np.pi * float(np.linalg.norm(SRC - MIC)))
    assert 0 < n < 200 and np.abs(a).max() <= M
    assert np.abs(a - b).max() <= n * n * 2.0 ** -52 * M
    with pytest.raises(ValueError, match='srate'):
        R.rir(ROOM, SRC, MIC, [0.5] * 6, 100, 44100)


def test_fixture_is_what_its_recipe_makes(rfx):
    assert list(rfx['rows']) == list(GR.ROWS) and rfx['meta']['margin_floor'] == GR.MARGIN
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'rir.pt')) < 1 << 20
    for name, row in GR.ROWS.items():
        c = rfx['rows'][name]
        assert np.array_equal(c['geom'].numpy(), GR.geom_of(row))
        assert (c['T'], c['srate'], c['length']) == tuple(row[4:])
        assert c['margin'] >= GR.MARGIN and c['h'].shape == (c['T'],)
        assert c['move'] <= 1e-13 * c['peak']
        if c['T'] <= 600:           # the short rows are run again here
            # numpy's sin and cos may round differently on another host: a different
            # implementation, held to the bound of the device, 100 x the row's movement
            o = R.rir_rows(c['geom'].numpy()[None], c['T'], c['srate'], [c['length']])
            assert np.abs(o['h'][0] - c['h'].numpy()).max() <= 100 * c['move']
            assert int(o['images'][0]) == c['images']
    rows = rfx['rows']
    assert rows['T1']['images'] == 0 and not rows['T1']['h'].any()
    assert not rows['masked']['h'][333:].any() and rows['masked']['h'][:333].abs().max() > 0
    assert rows['T2048']['images'] > 6000 and rows['small_live']['images'] > 11000
    assert torch.equal(rows['T255']['h'], rows['T256']['h'][:255]) or (
        rows['T255']['h'] - rows['T256']['h'][:255]).abs().max() < 1e-16


# ---- rooms --------------------------------------------------------------------------------------

def test_beta_from_rt60_against_hand_values():
    from segan_pytorch_amd.augment import beta_from_rt60
    # 5 x 4 x 3 m: V = 60, S = 94; 24 ln 10 / 343 = 0.161114...; absorption = 0.161114 * 60 / 28.2
    assert abs(float(beta_from_rt60([5, 4, 3], 0.3)) - np.sqrt(1 - 0.1611140 * 60 / 28.2)) < 1e-6
    assert abs(float(beta_from_rt60([5, 4, 3], 0.3)) - 0.81068) < 1e-5
    assert float(beta_from_rt60([5, 4, 3], 0.05)) == 0.0            # more absorption than walls
    b = beta_from_rt60([[5, 4, 3], [8, 6, 3.5]], [0.3, 0.5])
    assert b.shape == (2,) and b[1] == beta_from_rt60([8, 6, 3.5], 0.5)
    assert np.all(np.diff(beta_from_rt60([5, 4, 3], np.array([0.2, 0.4, 0.8]))) > 0)
    for bad in (([5, 4], 0.3), ([5, 4, 0], 0.3), ([5, 4, 3], 0.0)):
        with pytest.raises(ValueError, match='beta_from_rt60'):
            beta_from_rt60(*bad)


def test_draw_rooms_is_deterministic_and_keeps_its_margins():
    from segan_pytorch_amd.augment import beta_from_rt60, draw_rooms
    a = draw_rooms(np.random.default_rng(5), 200)
    b = draw_rooms(np.random.default_rng(5), 200)
    assert sorted(a) == ['beta', 'mic', 'room', 'rt60', 'src']
    for k in a:
        assert np.array_equal(a[k], b[k]) and a[k].dtype == np.float64
    # the first room does not depend on how many follow
    assert np.array_equal(draw_rooms(np.random.default_rng(5), 1)['mic'][0], a['mic'][0])
    assert not np.array_equal(draw_rooms(np.random.default_rng(6), 1)['room'][0], a['room'][0])
    assert np.all(a['room'] >= [3, 3, 2.5]) and np.all(a['room'] <= [10, 8, 4])
    assert np.all((a['rt60'] >= 0.2) & (a['rt60'] <= 0.8))
    for p in (a['src'], a['mic']):
        assert np.all(p >= 0.5) and np.all(p <= a['room'] - 0.5)
    assert np.all(np.sqrt(((a['src'] - a['mic']) ** 2).sum(axis=1)) >= 0.5)
    assert a['beta'].shape == (200, 6)
    assert np.array_equal(a['beta'][:, 0], beta_from_rt60(a['room'], a['rt60']))
    assert np.all(a['beta'] == a['beta'][:, :1])
    # a min_dist that is often missed is still kept, by drawing again
    far = draw_rooms(np.random.default_rng(7), 50, min_dist=2.0, room_min=(4, 4, 3))
    assert np.all(np.sqrt(((far['src'] - far['mic']) ** 2).sum(axis=1)) >= 2.0)
    tight = draw_rooms(np.random.default_rng(8), 20, rt60=(0.3, 0.3), room_min=(4, 4, 3),
                       room_max=(4, 4, 3), wall_margin=1.0)
    assert np.all(tight['rt60'] == 0.3) and np.all(tight['room'] == [4, 4, 3])
    assert np.all(tight['src'] >= 1.0) and np.all(tight['mic'] <= [3, 3, 2])
    for kw in (dict(count=0), dict(rt60=(0.5, 0.2)), dict(room_min=(11, 3, 2.5)),
               dict(wall_margin=1.5), dict(min_dist=9.0), dict(rt60=(0.0, 0.2))):
        with pytest.raises(ValueError, match='draw_rooms'):
            draw_rooms(np.random.default_rng(0), **dict(dict(count=2), **kw))


def test_there_is_no_cpu_path():
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import RIRBank
    if not torch.cuda.is_available():     # where a device is visible the call is the GPU test's
        for fn in (ops.rir_shoebox, ops.rir_stages):
            with pytest.raises(RuntimeError, match='MI355X'):
                fn(ROOM, SRC, MIC, [0.5] * 6, 64)
    with pytest.raises(RuntimeError, match='MI355X'):
        RIRBank.synthetic(2, seed=0, device='cpu')


def test_ops_argument_checks_raise_before_any_launch():
    from segan_pytorch_amd import ops
    ok = dict(room=ROOM, src=SRC, mic=MIC, beta=[0.5] * 6, taps=64)
    for bad in (dict(room=[5, 4]), dict(src=np.zeros((2, 2))), dict(beta=[0.5] * 5),
                dict(mic=np.zeros((2, 3, 1))), dict(room=np.ones((2, 3)), src=np.ones((3, 3)))):
        with pytest.raises(ValueError, match='rir: '):
            ops.rir_shoebox(**dict(ok, **bad))
    for bad in (0, -1, 1.5, True, ops.RIR_MAX_T + 1):
        with pytest.raises(ValueError, match='taps'):
            ops.rir_shoebox(**dict(ok, taps=bad))
    for bad in (0, 44100, 16000.5, True, None):
        with pytest.raises(ValueError, match='srate'):
            ops.rir_shoebox(**dict(ok, srate=bad))
    with pytest.raises(ValueError, match='n_max'):
        ops.rir_tables([0.5] * 6, -1)


# ---- header, binding, Makefile, library ---------------------------------------------------------

def test_binding_header_and_makefile_pins():
    from segan_pytorch_amd import _lib, ops
    assert len(_lib.SIGNATURES) == 119 and _lib.ABI_VERSION == 17
    assert list(_lib.EXT_SIGNATURES) == ['segan_wpe_dims', 'segan_wpe']
    assert list(_lib.PYIN_SIGNATURES) == ['segan_pyin_tables', 'segan_pyin_dims', 'segan_pyin']
    assert list(_lib.OMLSA_SIGNATURES) == ['segan_omlsa_dims', 'segan_omlsa']
    assert list(_lib.RIR_SIGNATURES) == ['segan_rir_dims', 'segan_rir']
    assert [len(_lib.RIR_SIGNATURES[n][1]) for n in _lib.RIR_SIGNATURES] == [4, 10]
    assert dict(_lib.RIR_DEFINES) == {'SEGAN_RIR_TILE': 256, 'SEGAN_RIR_GEOM': 15,
                                      'SEGAN_RIR_MAX_T': 1 << 20}
    assert (ops.RIR_TILE, ops.RIR_GEOM, ops.RIR_MAX_T, ops.RIR_C) == (256, 15, 1 << 20, R.C)
    assert tuple(ops.RIR_RATES) == tuple(R.RATES)
    assert not set(_lib.RIR_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES) |
                                           set(_lib.PYIN_SIGNATURES) | set(_lib.OMLSA_SIGNATURES))
    with pytest.raises(RuntimeError, match='not found'):
        _lib._read_header_file(_lib.RIR_HEADER_PATH + '.missing')
    with open(_lib.RIR_HEADER_PATH) as f:
        text = f.read()
    assert 'SEGAN_ABI_VERSION stays 17' in text and 'purely additive' in text
    assert 'SEGAN_ABI_VERSION' not in _lib.RIR_DEFINES
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    assert lib.segan_rir.argtypes == _lib.RIR_SIGNATURES['segan_rir'][1]
    assert lib.segan_rir_dims.restype is ctypes.c_int and lib.segan_rir.restype is ctypes.c_int
    with open(os.path.join(ROOT, 'Makefile')) as f:
        mk = f.read()
    assert '$(CSRC)/segan_rir.hip' in mk.split('SRCS :=')[1].split('\n')[0]
    rule = [l for l in mk.split('\n') if l.startswith('$(CSRC)/%.o:')][0]
    assert 'include/segan_rir.h' in rule and 'include/segan_omlsa.h' in rule
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        doc = f.read()
    assert 'segan_rir.h' in doc and 'segan_rir_dims' in doc and 'segan_rir(' in doc


def test_dims_and_checks_before_any_launch():
    from segan_pytorch_amd import _lib, ops
    lib = _lib.load()
    for srate in (16000, 8000):
        Hw = srate // 250
        for T in (1, 255, 256, 257, 16384, 1 << 20):
            d = ops.rir_dims(3, T, srate)
            tiles = (T + 255) // 256
            # a room of 1 m: |n| <= dhi / 2 + 2 and |n - q| one more
            dhi = (tiles * 256 + Hw + 1) * R.C / srate
            assert d == dict(half_width=Hw, stride=int(np.floor(dhi / 2.0)) + 4, tiles=tiles,
                             ws_bytes=3 * 15 * 8 + 3 * tiles * 8), (T, srate)
            assert Hw == R.half_width(srate)
    one = ctypes.c_void_p(16)     # never dereferenced: the arguments are refused first
    out = (ctypes.c_int64 * 4)()
    good = np.concatenate([ROOM, SRC, MIC, [0.5] * 6])

    def call(geom=good, tables=one, count=1, T=64, srate=16000, h=one, images=None, ws=one):
        g = None if geom is None else np.ascontiguousarray(geom, np.float64)
        return lib.segan_rir(None if g is None else g.ctypes.data_as(ctypes.c_void_p), tables, None,
                             count, T, srate, h, images, ws, None)

    for count, T, srate in ((0, 64, 16000), (65536, 64, 16000), (1, 0, 16000),
                            (1, (1 << 20) + 1, 16000), (1, 64, 44100), (1, 64, 0)):
        assert lib.segan_rir_dims(count, T, srate, out) != 0
        assert lib.segan_last_error().startswith(b'rir: bad sizes')
        assert call(count=count, T=T, srate=srate) != 0
        assert lib.segan_last_error().startswith(b'rir: bad sizes')
        with pytest.raises(RuntimeError, match='rir: bad sizes'):
            ops.rir_dims(count, T, srate)
    assert lib.segan_rir_dims(1, 64, 16000, None) != 0
    assert lib.segan_last_error().startswith(b'rir: NULL')
    for kw in (dict(geom=None), dict(tables=None), dict(h=None), dict(ws=None)):
        assert call(**kw) != 0 and lib.segan_last_error().startswith(b'rir: NULL'), kw
    for kw in (dict(tables=ctypes.c_void_p(12)), dict(h=ctypes.c_void_p(20)),
               dict(ws=ctypes.c_void_p(4)), dict(images=ctypes.c_void_p(2))):
        assert call(**kw) != 0 and lib.segan_last_error().startswith(b'rir: a pointer'), kw

    def geom(**kw):
        g = good.copy()
        for k, v in kw.items():
            g[int(k[1:])] = v
        return g

    for g, msg in ((geom(g0=0.99), b'not in 1 .. 50'), (geom(g1=50.5), b'not in 1 .. 50'),
                   (geom(g2=float('nan')), b'not in 1 .. 50'), (geom(g3=0.0), b'strictly inside'),
                   (geom(g4=4.0), b'strictly inside'), (geom(g8=3.5), b'strictly inside'),
                   (geom(g6=float('nan')), b'strictly inside'),
                   (geom(g6=SRC[0], g7=SRC[1], g8=SRC[2] + 0.049), b'below 0.05'),
                   (geom(g9=-0.01), b'beta 0'), (geom(g14=1.01), b'beta 5'),
                   (geom(g11=float('nan')), b'beta 2')):
        assert call(geom=g) != 0
        err = lib.segan_last_error()
        assert err.startswith(b'rir: room 0') and msg in err, (g, err)
    two = np.stack([good, geom(g9=2.0)])
    assert call(geom=two, count=2) != 0 and lib.segan_last_error().startswith(b'rir: room 1')


# ---- train.py and scripts/synth_rirs.py ---------------------------------------------------------

def test_train_flags():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.reverb_synth == 0 and d.reverb_rt60 == [0.2, 0.8]
    assert d.reverb_room_min == [3.0, 3.0, 2.5] and d.reverb_room_max == [10.0, 8.0, 4.0]
    assert train.check_reverb_flags(d) is False
    sh = ['--pcm_shard', 'sh']
    for argv in (['--reverb_synth', '8'], ['--reverb_synth', '8', '--reverb_rirs', 'dir'],
                 ['--reverb_synth', '8', '--reverb_prob', '0.5', '--reverb_max_taps', '4000'],
                 ['--reverb_synth', '8', '--reverb_rirs', 'dir', '--reverb_resample'],
                 ['--reverb_synth', '8', '--reverb_rt60', '0.3', '0.3', '--reverb_room_min', '2',
                  '2', '2', '--reverb_room_max', '50', '50', '50']):
        assert train.check_reverb_flags(p.parse_args(sh + argv)) is True, argv
    for bad, msg in (
            (['--reverb_synth', '8'], '--reverb_synth reverberates .* only together with --pcm_shard'),
            (['--reverb_synth', '8', '--synthetic', '8'], 'only together with'),
            (sh + ['--reverb_synth', '-1'], 'must not be negative'),
            (sh + ['--reverb_rt60', '0.2', '0.5'], 'need --reverb_synth N'),
            (sh + ['--reverb_rirs', 'd', '--reverb_room_min', '4', '4', '3'], 'need --reverb_synth'),
            (sh + ['--reverb_room_max', '9', '9', '3'], 'need --reverb_synth N'),
            (sh + ['--reverb_synth', '8', '--reverb_resample'], 'needs --reverb_rirs DIR'),
            (sh + ['--reverb_synth', '8', '--reverb_prob', '1.5'], 'must lie in 0 .. 1'),
            (sh + ['--reverb_synth', '8', '--reverb_max_taps', '0'], 'must be positive'),
            (sh + ['--reverb_synth', '8', '--reverb_rt60', '0.5', '0.2'], '0 < LO <= HI'),
            (sh + ['--reverb_synth', '8', '--reverb_rt60', '0', '0.2'], '0 < LO <= HI'),
            (sh + ['--reverb_synth', '8', '--reverb_room_min', '1', '3', '3'], 'metres per side'),
            (sh + ['--reverb_synth', '8', '--reverb_room_max', '2', '8', '4'], 'metres per side'),
            (sh + ['--reverb_synth', '8', '--reverb_room_max', '10', '8', '51'], 'metres per side')):
        with pytest.raises(SystemExit, match=msg):
            train.check_reverb_flags(p.parse_args(bad))
        with pytest.raises(SystemExit, match=msg):      # before anything touches a device
            train.main(p.parse_args(bad))
    # without the new flags every exit is worded as before
    for bad, msg in ((['--reverb_rirs', 'dir'],
                      '--reverb_rirs reverberates the batches of a pcm16 shard on the GPU: it is '
                      'valid only together with --pcm_shard PREFIX'),
                     (sh + ['--reverb_prob', '0.5'],
                      '--reverb_prob / --reverb_max_taps need --reverb_rirs DIR'),
                     (sh + ['--reverb_max_taps', '100'],
                      '--reverb_prob / --reverb_max_taps need --reverb_rirs DIR'),
                     (sh + ['--reverb_resample'], '--reverb_resample needs --reverb_rirs DIR'),
                     (sh + ['--reverb_rirs', 'd', '--reverb_prob', '1.5'],
                      '--reverb_prob must lie in 0 .. 1, got 1.5'),
                     (sh + ['--reverb_rirs', 'd', '--reverb_max_taps', '0'],
                      '--reverb_max_taps must be positive, got 0')):
        with pytest.raises(SystemExit) as e:
            train.check_reverb_flags(p.parse_args(bad))
        assert str(e.value) == msg
    assert '--reverb_synth' in train.__doc__ and '--reverb_rt60' in train.__doc__


def test_synth_rirs_cli():
    import synth_rirs as S
    from segan_pytorch_amd.augment import draw_rooms
    p = S.build_parser()
    o = p.parse_args(['--out', 'd', '--count', '3', '--seed', '4'])
    assert (o.srate, o.max_taps, o.rt60, o.wall_margin, o.min_dist) == (16000, 16384, [0.2, 0.8],
                                                                        0.5, 0.5)
    assert o.room_min == [3.0, 3.0, 2.5] and o.room_max == [10.0, 8.0, 4.0]
    for argv in ([], ['--out', 'd', '--count', '3'], ['--out', 'd', '--count', '3', '--seed', '0',
                                                      '--srate', '44100']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)
    for argv, msg in ((['--count', '0'], 'count'), (['--count', '10000'], 'count'),
                      (['--count', '3', '--max_taps', '0'], 'max_taps')):
        with pytest.raises(SystemExit, match=msg):
            S.main(p.parse_args(['--out', 'd', '--seed', '0'] + argv))
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match='MI355X'):
            S.main(o)
    rooms = draw_rooms(np.random.default_rng(4), 3)
    rows = S.rows_of(rooms, [100, 200, 300])
    assert [r[0] for r in rows] == ['rir_0000.wav', 'rir_0001.wav', 'rir_0002.wav']
    assert all(len(r) == len(S.COLUMNS) for r in rows) and rows[1][1] == '200'
    assert float(rows[2][2]) == rooms['rt60'][2] and float(rows[0][12]) == rooms['mic'][0, 2]
    assert float(rows[1][3]) == rooms['beta'][1, 0] and float(rows[1][4]) == rooms['room'][1, 0]
