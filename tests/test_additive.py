"""Host side of the additive-noise mixer: the numpy oracle against the
fixture computed by the real reference (tests/golden/additive.pt, recipe
scripts/make_golden_additive.py), the dilation form of the hangover counts against the literal
loop, NoiseBank and the draws, the train.py flags, the segan.utils names and the C ABI: no GPU."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import additive_oracle as A  # noqa: E402
import make_golden_additive as G  # noqa: E402

CASES = ('ord16k', 'ord40k', 'quiet', 'low', 'zeros', 'zero_run', 'extreme', 'clip', 'short', 'sr8k')


@pytest.fixture(scope='module')
def afx():
    return load_golden('additive.pt')


@pytest.fixture(scope='module')
def noises():
    return G.noise_bank()


def _rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def test_fixture_holds_the_required_cases(afx, noises):
    assert set(afx['cases']) == set(CASES)
    assert [G.sha(d) for d in noises] == afx['noise_sha']
    T = afx['truth']
    assert T['zeros']['counts'][0] == 0 and math.isnan(T['zeros']['c0'])
    assert T['low']['counts'][0] > 0 and math.isnan(T['low']['c0']) and T['low']['asl_ms'] == 0
    assert T['extreme']['shortcut'] and T['extreme']['c0'] == 2.0 ** -8
    assert T['clip']['n'] >= 1
    assert {afx['cases'][k]['T'] for k in CASES} >= {16384, 40000, 77}
    assert afx['cases']['sr8k']['srate'] == 8000
    z = afx['cases']['zero_run']['zero']
    assert z[1] - z[0] > 2 * 16000
    for k in CASES:      # no fixture sits on a knife edge
        assert afx['margins'][k]['q'] > 1e-9 and afx['margins'][k]['interp_db'] > 1e-6, k


@pytest.mark.parametrize('name', CASES)
def test_oracle_reproduces_the_reference(afx, noises, name):
    rc, t = afx['cases'][name], afx['truth'][name]
    x = G.case_signal(rc)
    assert G.sha(x) == afx['sha'][name]['signal']
    got = A.asl_p56(x, rc['srate'])
    assert got['counts'].tolist() == t['counts'].tolist()
    assert got['status'] == 0
    for k in ('sq', 'asl_ms', 'asl'):
        assert _rel(got[k], t[k]) <= 1e-12, (k, got[k], t[k])
    if math.isnan(t['c0']):
        assert got['c0'] is None and got['asl_ms'] == 0 and got['asl'] == 0
    else:
        assert _rel(got['c0'], t['c0']) <= 1e-12
    if name in afx['q']:
        want = afx['q'][name].numpy()
        assert np.abs(got['q'] - want).max() <= 1e-12 * want.max()
    seg = noises[t['noise_idx']][t['start']:t['start'] + rc['T']]
    m = A.mix(x, seg, t['snr'], t['asl_ms'])
    assert m['n'] == t['n']
    assert _rel(m['Pn'], t['Pn']) <= 1e-12 and _rel(m['sf'], t['sf']) <= 1e-12
    want32 = G.truth_mix(x, seg, t['sf'], t['n']).astype(np.float32)
    assert G.sha(want32) == afx['sha'][name]['noisy32']      # what the reference returned
    ulps = np.abs(m['noisy32'].view(np.int32).astype(np.int64) - want32.view(np.int32))
    assert ulps.max() <= 1
    if t['asl_ms'] == 0:
        assert np.array_equal(m['noisy32'], x)
    if name == 'short':
        assert np.array_equal(want32, afx['short_noisy32'].numpy())


def test_dilation_counts_equal_the_literal_hangover_loop():
    """a_j = |exceedance set dilated I samples to the right|, on short signals at 1 kHz (I = 200):
    bursts separated by zero runs shorter and longer than the hangover, very low levels, a
    signal that starts active, an all-zero one."""
    rng = np.random.default_rng(5)
    sr, n = 1000, 3000
    sigs = []
    for lvl in (0.5, 0.01, 2e-4):
        x = rng.standard_normal(n) * lvl
        x[400:520] = 0          # shorter than the hangover
        x[900:1500] = 0         # longer
        x[2100:2350] = 0
        sigs.append(x)
    ramp = np.linspace(0, 1, n) ** 3 * rng.standard_normal(n) * 0.3
    sigs += [ramp, ramp[::-1].copy(), np.zeros(n), np.r_[np.zeros(2900), 0.5 * np.ones(100)]]
    for i, x in enumerate(sigs):
        q = A.envelope(x, sr)
        fast, loop = A.activity_counts(q, sr), A.activity_counts_loop(q, sr)
        assert fast.tolist() == loop.tolist(), i
    assert A.activity_counts(A.envelope(sigs[0], sr), sr)[0] > 0
    assert A.hangover(16000) == 3200 and A.hangover(8000) == 1600 and A.hangover(11025) == 2205


def test_bin_interp_cap_reports_instead_of_spinning():
    assert A.bin_interp(float('nan'), 1.0, 2.0, 3.0, 15.9, 0.5)[2] == 1
    assert A.clip_divisions(0.5, -0.5) == 0 and A.clip_divisions(1.0, 0.0) == 1
    assert A.clip_divisions(0.0, -1.0) == 0 and A.clip_divisions(1.1 * 1.2 * 1.01, 0.0) == 3


# ---- NoiseBank, draws, Additive ---------------------------------------------------------------

def test_noise_bank_concatenates_with_offsets(tmp_path):
    from segan_pytorch_amd.augment import NoiseBank
    a = np.arange(5, dtype=np.int16) * 1000
    b = np.linspace(-1, 1, 7).astype(np.float64)
    nb = NoiseBank([a, torch.from_numpy(b)])
    assert len(nb) == 2 and nb.offsets.tolist() == [0, 5, 12] and nb.lengths.tolist() == [5, 7]
    assert nb.host.dtype == np.float32
    assert np.array_equal(nb.host[:5], a.astype(np.float32) / np.float32(32768))
    assert np.array_equal(nb.host[5:], b.astype(np.float32))
    with pytest.raises(TypeError):
        NoiseBank([np.arange(4, dtype=np.int32)])
    with pytest.raises(ValueError, match='No noises found'):
        NoiseBank([])
    with pytest.raises(RuntimeError, match='MI355X'):
        nb.data('cpu')
    wavfile.write(str(tmp_path / 'b.wav'), 16000, (np.arange(10) - 5).astype(np.int16))
    wavfile.write(str(tmp_path / 'a.wav'), 16000, (np.arange(6) * 100).astype(np.int16))
    fd = NoiseBank.from_dir(str(tmp_path))
    assert [os.path.basename(f) for f in fd.files] == ['a.wav', 'b.wav']
    assert fd.offsets.tolist() == [0, 6, 16]
    assert np.array_equal(fd.host[:6], (np.arange(6) * 100).astype(np.float32) / np.float32(32768))


def test_empty_noise_directory_raises_the_reference_message(tmp_path):
    from segan_pytorch_amd.augment import Additive, NoiseBank
    msg = re.escape('[!] No noises found in {}'.format(tmp_path))
    with pytest.raises(ValueError, match=msg):
        NoiseBank.from_dir(str(tmp_path))
    with pytest.raises(ValueError, match=msg):
        Additive(str(tmp_path))


def test_draws_are_valid_uniform_and_repeatable():
    from segan_pytorch_amd.augment import NoiseBank
    nb = NoiseBank([np.ones(12, np.float32), np.ones(30, np.float32)])
    ids, sn, st = nb.draw(np.random.default_rng(3), [10] * 400, [0, 5, 10])
    assert set(ids.tolist()) == {0, 1} and set(sn.tolist()) == {0.0, 5.0, 10.0}
    # valid starts 1 .. len - T: both ends are drawn, nothing outside, no segment leaves its file
    assert set(st[ids == 0].tolist()) == {1, 2}
    assert set(st[ids == 1].tolist()) == set(range(1, 21))
    assert (st + 10 <= nb.lengths[ids]).all() and (st >= 1).all()
    again = nb.draw(np.random.default_rng(3), [10] * 400, [0, 5, 10])
    assert all(np.array_equal(a, b) for a, b in zip((ids, sn, st), again))
    other = nb.draw(np.random.default_rng(4), [10] * 400, [0, 5, 10])
    assert not np.array_equal(other[2], st)
    # given values are kept, the rest is drawn
    ids2, sn2, st2 = nb.draw(np.random.default_rng(3), [10, 10], [0, 5], noise_ids=[1, 1],
                             snrs=[7.5, -3], starts=[20, 1])
    assert ids2.tolist() == [1, 1] and sn2.tolist() == [7.5, -3.0] and st2.tolist() == [20, 1]
    with pytest.raises(ValueError, match='outside 1 .. 20'):
        nb.draw(np.random.default_rng(3), [10], [0], noise_ids=[1], starts=[21])
    with pytest.raises(ValueError, match='pass noise_ids'):
        nb.draw(np.random.default_rng(3), [10], [0], starts=[1])
    with pytest.raises(ValueError, match='Noise length has to be greater than speech length'):
        nb.draw(np.random.default_rng(3), [12], [0], noise_ids=[0])
    with pytest.raises(ValueError, match='Noise length has to be greater than speech length'):
        NoiseBank([np.ones(8, np.float32)]).draw(np.random.default_rng(0), [9], [0])


def test_additive_object_and_the_segan_utils_names(noises):
    import segan.utils as U
    from segan_pytorch_amd import augment, ops
    assert U.Additive is augment.Additive and U.ComposeAdditive is augment.ComposeAdditive
    from segan.utils import Additive, ComposeAdditive, CompositeEval  # noqa: F401
    sig = inspect.signature(U.Additive.__init__)
    assert list(sig.parameters)[:4] == ['self', 'noises', 'snr_levels', 'do_IRS']
    assert sig.parameters['snr_levels'].default == [0, 5, 10]
    assert sig.parameters['do_IRS'].default is False
    assert list(inspect.signature(U.Additive.__call__).parameters) == ['self', 'wav', 'srate', 'nbits']
    with pytest.raises(NotImplementedError):
        U.Additive(noises, do_IRS=True)
    add = U.Additive(noises, snr_levels=[0, 5], seed=1)
    assert add.snr_levels == [0, 5] and len(add.bank) == 2
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='MI355X'):
            add(np.zeros(100, np.float32))
        pair = U.ComposeAdditive(lambda x: x + 1)(np.zeros(3))
        assert pair[0].tolist() == [0, 0, 0] and pair[1].tolist() == [1, 1, 1]
    x = torch.zeros(2, 64)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.asl_p56(x)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.additive_mix(x, torch.zeros(100), [1, 1], [0, 0], torch.zeros(2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='MI355X'):
        add.mix(x)


# ---- train.py flags ---------------------------------------------------------------------------

def test_train_flags_parse_and_go_with_pcm_shard():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.additive_noises is None and d.additive_snrs == [0, 5, 10] and d.additive_prob == 1.0
    assert train.check_additive_flags(d) is False
    o = p.parse_args(['--pcm_shard', 'sh', '--additive_noises', 'dir', '--additive_snrs', '-5',
                      '2.5', '--additive_prob', '0.25'])
    assert o.additive_snrs == [-5.0, 2.5] and o.additive_prob == 0.25
    assert train.check_additive_flags(o) is True
    for bad, msg in ((['--additive_noises', 'dir'], 'only together with --pcm_shard'),
                     (['--additive_noises', 'dir', '--synthetic', '8'], 'only together with'),
                     (['--pcm_shard', 'sh', '--additive_snrs', '3'], 'need --additive_noises'),
                     (['--pcm_shard', 'sh', '--additive_prob', '0.5'], 'need --additive_noises'),
                     (['--pcm_shard', 'sh', '--additive_noises', 'd', '--additive_prob', '1.5'],
                      'must lie in 0 .. 1')):
        with pytest.raises(SystemExit, match=msg):
            train.check_additive_flags(p.parse_args(bad))
        with pytest.raises(SystemExit, match=msg):      # before anything touches a device
            train.main(p.parse_args(bad))


def test_loader_checks_the_probability():
    from segan_pytorch_amd.datasets import PCMShardLoader
    with pytest.raises(ValueError, match='additive_prob'):
        PCMShardLoader(None, 2, 0.95, 'cpu', additive=object(), additive_prob=1.5)


# ---- C ABI -------------------------------------------------------------------------------------

def test_header_lib_and_abi_agree():
    from segan_pytorch_amd import _lib
    assert H.macro('SEGAN_ABI_VERSION') == 17
    assert _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    for name in ('segan_asl_p56', 'segan_additive_mix', 'segan_pcm16_wave', 'segan_preemph_rows'):
        assert len(H.args(name)) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert 'segan_asl_p56' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    # arguments are validated before any launch
    assert lib.segan_asl_p56(None, None, 1, 16, 16000, 16, None, None, None, None, None) == -1
    assert b'asl_p56' in lib.segan_last_error()
    buf = torch.zeros(64, dtype=torch.float64)
    p = buf.data_ptr()
    assert lib.segan_asl_p56(p, None, 1, 16, 16000, 8, p, p, p, None, None) == -3
    assert b'nbits=8' in lib.segan_last_error()
    assert lib.segan_asl_p56(p, None, 1, 0, 16000, 16, p, p, p, None, None) == -1
    assert lib.segan_additive_mix(p, None, p, 0, p, p, p, None, 1, 16, p, None, p, p, None) == -1
    assert lib.segan_additive_mix(p, None, p, 64, p, p, p, p, 1, 16, p, None, p, p, None) == -1
    assert b'prev' in lib.segan_last_error()
