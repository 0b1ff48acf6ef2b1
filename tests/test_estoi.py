"""Host side of ESTOI (the numpy oracle scripts/estoi_oracle.py, the fixture tests/golden/estoi.pt,
the CLI flags, the additive C ABI entry): no GPU."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import estoi_oracle as E  # noqa: E402
import make_golden_estoi as GE  # noqa: E402

# ESTOI of stoi.pt's cases by the rules of DESIGN.md section 10, numpy fp64 (the issue's table)
TABLE = {'snrm5': 0.371545247265, 'snr0': 0.469522558517, 'snr10': 0.654013684897,
         'odd_len': 0.654013684897, 'snr20': 0.881272092328, 'scaled': 1.0,
         'zero_run': 0.198284628811, 'sr10k': 0.343016614073, 'sr8k': 0.423392381041,
         'sr44k': 0.925655190625, 'stage16k': 0.443896434830, 'stage8k': 0.505374061104,
         'short': math.nan, 'silent': math.nan}


@pytest.fixture(scope='module')
def sfx():
    return load_golden('stoi.pt')


@pytest.fixture(scope='module')
def efx():
    return load_golden('estoi.pt')


@pytest.fixture(scope='module')
def stages(sfx, efx):
    """The oracle's stages of every case, computed once."""
    return {name: E.estoi_stages(*GE.case_signals(sfx, efx, name)) for name in efx['d']}


def test_oracle_reproduces_the_fixture(sfx, efx, stages):
    assert set(efx['d']) == set(sfx['cases']) | {'m30', 'm31', 'm32'}
    assert set(efx['dm']) == {'stage16k', 'stage8k', 'zero_run', 'm31', 'm32'}
    for name, want in efx['d'].items():
        got = stages[name]['d']
        if math.isnan(want):
            assert math.isnan(got), name
        else:
            assert abs(got - want) <= 1e-12, (name, got, want)
    assert [n for n, v in efx['d'].items() if math.isnan(v)] == ['short', 'silent', 'm30']
    for name, want in efx['dm'].items():
        got = stages[name]['dm']
        assert got.shape == tuple(want.shape) == (max(efx['M'][name] - 30, 0),)
        assert np.abs(got - want.numpy()).max() <= 1e-12, name


def test_oracle_reproduces_the_table(efx, stages):
    assert set(TABLE) == set(efx['d']) - {'m30', 'm31', 'm32'}
    for name, want in TABLE.items():
        got = stages[name]['d']
        if math.isnan(want):
            assert math.isnan(got), name
        else:
            assert abs(got - want) <= 1e-9, (name, got, want)


def test_short_slices_have_no_one_and_two_segments(sfx, efx, stages):
    rcs = efx['extra_cases']
    assert {n: rc['len'] for n, rc in rcs.items()} == {'m30': 9856, 'm31': 10048, 'm32': 13568}
    for name, M in (('m30', 30), ('m31', 31), ('m32', 32)):
        rc = rcs[name]
        assert (rc['start'], rc['srate'], rc['gain']) == (8000, 16000,
                                                          sfx['cases']['stage16k']['gain'])
        assert stages[name]['M'] == efx['M'][name] == M
        assert stages[name]['dm'].shape == (M - 30,)
    assert math.isnan(stages['m30']['d'])
    assert stages['m31']['d'] == stages['m31']['dm'][0]


def test_identity_is_one_on_every_segment(sfx, efx):
    for name in ('snr0', 'sr8k', 'zero_run'):
        ref, _, sr = GE.case_signals(sfx, efx, name)
        st = E.estoi_stages(ref, ref, sr)
        assert st['dm'].size > 0 and np.abs(st['dm'] - 1).max() <= 1e-12, name
        assert abs(st['d'] - 1) <= 1e-12


def test_scaling_the_processed_signal_changes_nothing(sfx, efx, stages):
    for name in ('snr0', 'stage8k', 'zero_run'):
        ref, deg, sr = GE.case_signals(sfx, efx, name)
        got = E.estoi(ref, deg * np.float32(0.25), sr)
        assert abs(got - stages[name]['d']) <= 1e-12, name


@pytest.mark.parametrize('name,seg', [('stage16k', 0), ('stage16k', 13), ('zero_run', 40),
                                      ('zero_run', 70), ('m31', 0)])
def test_per_element_loops_agree_with_the_array_form(stages, name, seg):
    st = stages[name]
    X, Y = st['X'][:, seg:seg + 30], st['Y'][:, seg:seg + 30]
    assert X.shape == (15, 30)
    assert abs(E.segment_value_loops(X, Y) - st['dm'][seg]) <= 1e-13


def test_zero_rule_margin_holds_on_every_case(efx, stages):
    """No e / raw in [2^-80, 2^-20]: the threshold 2^-40 sits in a gap, so the kernel's sums, in
    another order, take the oracle's keep / drop decisions."""
    assert E.ZERO_RULE == 2.0 ** -40 and E.MARGIN == (2.0 ** -80, 2.0 ** -20)
    for name, st in stages.items():
        r = st['ratios']
        assert E.margin_ok(r), name
        assert not np.any((r >= 2.0 ** -80) & (r <= 2.0 ** -20)), name
        kept, dropped = efx['ratio_gap'][name]
        assert kept > 2.0 ** -20 and dropped < 2.0 ** -80
        if name != 'zero_run':
            assert st['zeroed'] == 0 and dropped == 0
    z = efx['zero_run']
    assert stages['zero_run']['zeroed'] == z['zeroed'] > z['dropped_with_energy'] == 60
    assert z['largest_dropped'] <= 7.9e-32 and z['smallest_kept'] >= 5.4e-5
    assert not E.margin_ok(np.array([1.0, 2.0 ** -40]))


def test_zero_rule_on_degenerate_vectors():
    W = np.zeros((1, 15, 30))
    W[0, 0] = 3.0                                   # constant: no centred energy
    W[0, 1] = np.arange(30.0)                       # kept
    W[0, 2] = 1.0 + 1e-9 * np.arange(30.0)          # centred energy 7e-16 of raw, under 2^-40
    out, ratios, zeroed = E.normalise(W, 2)
    assert zeroed == 14 and ratios.size == 3
    assert not out[0, 0].any() and not out[0, 2].any() and not out[0, 3:].any()
    assert abs(np.sum(out[0, 1] ** 2) - 1) <= 1e-15 and abs(out[0, 1].sum()) <= 1e-15


def test_fixture_is_small_and_stores_no_signals(efx):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'estoi.pt'))
    assert size < 16 * 1024, size
    assert 'signals' not in efx and efx['meta']['signals'] == 'tests/golden/stoi.pt'
    assert len(efx['cli_d']) == 3 and all(math.isfinite(v) for v in efx['cli_d'].tolist())


def test_train_parses_eval_estoi():
    import train
    d = train.build_parser().parse_args([])
    assert d.eval_estoi is False and d.eval_stoi is False
    o = train.build_parser().parse_args(['--eval_estoi'])
    assert o.eval_estoi is True and o.eval_stoi is False


def test_eval_cli_parses_estoi():
    import eval_noisy_performance as ev
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    assert ev.build_parser().parse_args(req).estoi is False
    o = ev.build_parser().parse_args(req + ['--estoi'])
    assert o.estoi is True and o.stoi is False


def test_eval_cli_estoi_refuses_without_a_hip_device(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               ROCR_VISIBLE_DEVICES='-1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'eval_noisy_performance.py'),
                        '--test_wavs', str(tmp_path), '--clean_wavs', str(tmp_path),
                        '--logfile', str(tmp_path / 'log'), '--estoi'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env,
                       universal_newlines=True, timeout=300)
    assert p.returncode != 0
    assert 'runs only on an MI355X (HIP) device' in p.stdout, p.stdout
    assert not (tmp_path / 'log').exists()


def test_estoi_refuses_cpu_tensors():
    import torch
    from segan_pytorch_amd import ops, quality
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.estoi(x, x)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.estoi(x, x)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.estoi_stages(x, x)


def test_abi_entry_is_additive():
    from segan_pytorch_amd import _lib
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    assert re.search(r'\bint segan_estoi\(const float\* ref, const float\* deg, const int\* lengths', H.CODE)
    assert _lib.SIGNATURES['segan_estoi'] == _lib.SIGNATURES['segan_stoi']
    lib = _lib.load()
    assert lib.segan_abi_version() == 17 and hasattr(lib, 'segan_estoi')
    # arguments are checked before any launch: no device is needed to be refused
    assert lib.segan_estoi(*([None] * 3 + [1, 4000, 16000] + [None] * 13)) != 0
    assert b'estoi' in lib.segan_last_error()
    assert 'segan_estoi' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
