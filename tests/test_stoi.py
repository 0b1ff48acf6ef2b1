"""Host side of STOI (segan_stoi_plan, the numpy oracle, the fixture, the CLI flags): no GPU."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_stoi as G  # noqa: E402
import stoi_oracle as S  # noqa: E402


@pytest.fixture(scope='module')
def sfx():
    return load_golden('stoi.pt')


@pytest.mark.parametrize('srate', [16000, 8000, 44100])
def test_plan_taps_and_bands_match_the_fixture(sfx, srate):
    from segan_pytorch_amd import ops
    p, q, taps, bands = ops.stoi_plan(srate)
    want = sfx['plans'][srate]
    assert (p, q) == (want['p'], want['q'])
    assert taps.shape == want['taps'].shape
    assert (taps - want['taps']).abs().max().item() <= 1e-14 * want['taps'].abs().max().item()
    assert bands.tolist() == want['bands'].tolist()
    assert bands.tolist()[0] == [7, 9] and bands.tolist()[-1] == [174, 219]


def test_plan_at_10k_is_the_identity(sfx):
    from segan_pytorch_amd import ops
    p, q, taps, _ = ops.stoi_plan(10000)
    assert (p, q) == (1, 1) and taps.tolist() == [1.0]
    assert sfx['plans'][10000]['taps'].tolist() == [1.0]


def test_plan_rejects_rates_outside_4k_to_48k():
    from segan_pytorch_amd import ops
    for bad in (3999, 48001, 0, 16000.0, '16000', None):
        with pytest.raises(ValueError):
            ops.stoi_plan(bad)
    assert ops.stoi_plan(47999)[2].numel() == 2 * 10 * 47999 + 1


@pytest.mark.parametrize('srate', [11025, 37800])
def test_plan_keeps_the_index_order_sum_where_the_public_designer_compensates(srate):
    """STOI and ops.resample share one filter designer with two normalisation modes.  At these
    rates the public mode swaps the index-order sum of h for a compensated one, so its taps at
    (10, 5.0) are not STOI's bits; STOI's must stay the index-order ones its oracle pins.  Equal
    bits here would mean STOI has picked up the compensated mode.  The two stay within the
    rounding of a sequential fp64 sum of n terms, (n - 1) 2^-53 of the peak."""
    import torch
    from segan_pytorch_amd import ops
    staps = ops.stoi_plan(srate)[2]
    taps = ops.resample_plan(srate, 10000, 10, 5.0)[2]
    assert taps.shape == staps.shape
    diff = (taps - staps).abs().max().item()
    print(srate, 'max |stoi taps - public taps| = {:.3e}'.format(diff))
    assert not torch.equal(staps, taps)
    n, peak = taps.numel(), taps.max().item()
    assert diff <= (n - 1) * 2.0 ** -53 * peak


def test_oracle_reproduces_the_fixture(sfx):
    assert set(sfx['cases']) >= {'snrm5', 'snr0', 'snr10', 'snr20', 'scaled', 'zero_run', 'short',
                                 'silent', 'sr10k', 'sr8k', 'sr44k', 'odd_len', 'stage16k',
                                 'stage8k'}
    for name in sfx['cases']:
        ref, deg, sr = G.case_signals(sfx, name)
        got, want = S.stoi(ref, deg, sr), sfx['d'][name]
        if math.isnan(want):
            assert math.isnan(got), name
        else:
            assert abs(got - want) <= 1e-12, (name, got, want)
    assert math.isnan(sfx['d']['short']) and math.isnan(sfx['d']['silent'])
    assert sfx['zero_run_windows'] > 0


def test_oracle_resampling_equals_the_upfirdn_procedure(sfx):
    rng = np.random.default_rng(7)
    for sr in sfx['plans']:
        p, q, taps = S.plan(sr)
        for L in (1, 257, 4801, 9999):
            x = rng.standard_normal(L)
            a, b = S.resample(x, p, q, taps), S.resample_upfirdn(x, p, q, taps)
            assert a.shape == b.shape == (-(-L * p // q),)
            assert np.abs(a - b).max() <= 1e-13 * np.abs(x).max(), (sr, L)


def test_oracle_stage_shapes_follow_the_frame_rules(sfx):
    for name in ('stage16k', 'stage8k'):
        st = sfx['stages'][name]
        M = st['M']
        assert int(st['mask'].sum()) == M
        assert st['mask'].numel() == S.n_frames(st['xr'].numel())
        assert st['xs'].numel() == (M - 1) * S.K + S.N
        assert st['X'].shape == st['Y'].shape == (S.J, M - 1)
        assert st['rho'].shape == (M - 30, S.J)


def test_train_parses_eval_stoi():
    import train
    assert train.build_parser().parse_args([]).eval_stoi is False
    assert train.build_parser().parse_args(['--eval_stoi']).eval_stoi is True


def test_eval_cli_stoi_refuses_without_a_hip_device(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               ROCR_VISIBLE_DEVICES='-1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'eval_noisy_performance.py'),
                        '--test_wavs', str(tmp_path), '--clean_wavs', str(tmp_path),
                        '--logfile', str(tmp_path / 'log'), '--stoi'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env,
                       universal_newlines=True, timeout=300)
    assert p.returncode != 0
    assert 'runs only on an MI355X (HIP) device' in p.stdout, p.stdout
    assert not (tmp_path / 'log').exists()


def test_stoi_refuses_cpu_tensors():
    import torch
    from segan_pytorch_amd import ops, quality
    x = torch.zeros(2, 4000)
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.stoi(x, x)
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.stoi(x, x)
