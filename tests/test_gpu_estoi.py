"""ESTOI on the MI355X (ops.estoi / ops.estoi_stages, quality.estoi, SEGAN.evaluate with
eval_estoi, eval_noisy_performance.py --estoi) against the fp64 numpy oracle
(scripts/estoi_oracle.py -> tests/golden/estoi.pt, recipe scripts/make_golden_estoi.py; the
signals are tests/golden/stoi.pt's).  Tolerances are those of STOI's tests against its oracle."""
import math
import os
import stat
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
from make_golden_estoi import case_signals  # noqa: E402

pytestmark = pytest.mark.gpu

FRONT = ('xr', 'yr', 'energy', 'mask', 'xs', 'ys')     # written over their whole extent


@pytest.fixture(scope='module')
def sfx():
    return load_golden('stoi.pt')


@pytest.fixture(scope='module')
def efx():
    return load_golden('estoi.pt')


def _cuda(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda().unsqueeze(0) for a in arrs]


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def test_every_fixture_case(sfx, efx):
    from segan_pytorch_amd import ops
    worst_d = worst_dm = 0.0
    for name, want in efx['d'].items():
        ref, deg, sr = case_signals(sfx, efx, name)
        st = ops.estoi_stages(*_cuda(ref, deg), srate=sr)
        d = st['d']
        assert d.dtype == torch.float64 and d.shape == (1,)
        M = int(st['count'][0])
        assert M == efx['M'][name], name
        got = float(d[0])
        if math.isnan(want):
            assert math.isnan(got), (name, got)
        else:
            worst_d = max(worst_d, abs(got - want))
            assert abs(got - want) <= 1e-8, (name, got, want)
        if name in efx['dm']:
            dm = st['dm'][0, :max(M - 30, 0)].cpu()
            assert dm.shape == efx['dm'][name].shape and not torch.isnan(dm).any()
            worst_dm = max(worst_dm, (dm - efx['dm'][name]).abs().max().item())
            assert (dm - efx['dm'][name]).abs().max().item() <= 1e-7, name
    print('max |d - oracle| = {:.3e}, max |dm - oracle| = {:.3e}'.format(worst_d, worst_dm))
    assert set(efx['dm']) == {'stage16k', 'stage8k', 'zero_run', 'm31', 'm32'}


def test_slices_with_30_31_32_kept_frames_give_0_1_2_segments(sfx, efx):
    from segan_pytorch_amd import ops
    for name, M in (('m30', 30), ('m31', 31), ('m32', 32)):
        ref, deg, sr = case_signals(sfx, efx, name)
        st = ops.estoi_stages(*_cuda(ref, deg), srate=sr)
        assert int(st['count'][0]) == M
        dm = st['dm'][0, :M - 30].cpu()
        d = float(st['d'][0])
        if M == 30:
            assert math.isnan(d)
        else:
            assert dm.numel() == M - 30 == efx['dm'][name].numel()
            assert (dm - efx['dm'][name]).abs().max().item() <= 1e-7
            assert abs(d - efx['d'][name]) <= 1e-8
            assert abs(d - float(dm.sum()) / (M - 30)) <= 1e-15


def test_identity_and_scaling(sfx, efx):
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.quality import estoi
    ref, deg, _ = case_signals(sfx, efx, 'snr0')
    x, y = torch.from_numpy(ref).cuda(), torch.from_numpy(deg).cuda()
    st = ops.estoi_stages(x[None], x[None])
    S = int(st['count'][0]) - 30
    assert S > 0 and (st['dm'][0, :S] - 1).abs().max().item() <= 1e-12
    assert abs(float(estoi(x, x)[0]) - 1) <= 1e-12
    assert abs(float(estoi(x, x * 0.25)[0]) - 1) <= 1e-12
    assert abs(float(estoi(x, y * 0.25)[0]) - float(estoi(x, y)[0])) <= 1e-12


@pytest.mark.parametrize('name', ['stage16k', 'stage8k'])
def test_front_end_is_bitwise_stois(sfx, efx, name):
    from segan_pytorch_amd import ops
    ref, deg, sr = case_signals(sfx, efx, name)
    a = ops.stoi_stages(*_cuda(ref, deg), srate=sr)
    b = ops.estoi_stages(*_cuda(ref, deg), srate=sr)
    assert a['dims'] == b['dims'] and set(b) == (set(a) - {'rho'}) | {'dm'}
    assert b['dm'].shape == (1, a['dims'][4])
    for k in FRONT + ('count',):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    M = int(a['count'][0])
    assert torch.equal(a['kept'][0, :M].cpu(), b['kept'][0, :M].cpu())
    for k in ('X', 'Y'):
        assert torch.equal(_bits(a[k][0, :, :M - 1]), _bits(b[k][0, :, :M - 1])), k


def test_batch_with_lengths_is_bitwise_the_single_row_call(sfx, efx):
    from segan_pytorch_amd import ops
    names = ['stage16k', 'short', 'zero_run', 'silent', 'm31']
    sigs = [case_signals(sfx, efx, n)[:2] for n in names]
    lens = [len(r) for r, _ in sigs]
    assert len(set(lens)) >= 4
    T = max(lens)
    ref = np.zeros((len(sigs), T), np.float32)
    deg = np.full((len(sigs), T), 0.7, np.float32)   # junk past each row's length
    for i, (r, g) in enumerate(sigs):
        ref[i, :len(r)] = r
        deg[i, :len(g)] = g
    ref, deg = torch.from_numpy(ref).cuda(), torch.from_numpy(deg).cuda()
    st = ops.estoi_stages(ref, deg, 16000, lengths=lens)
    d = st['d']
    single = [ops.estoi_stages(*_cuda(r, g), srate=16000) for r, g in sigs]
    assert torch.equal(_bits(d), _bits(torch.cat([s['d'] for s in single])))
    assert torch.isnan(d.cpu()).tolist() == [False, True, False, True, False]
    for i, s in enumerate(single):
        S = max(int(s['count'][0]) - 30, 0)
        assert torch.equal(_bits(st['dm'][i, :S]), _bits(s['dm'][0, :S])), names[i]
    perm = [3, 0, 4, 2, 1]
    dp = ops.estoi(ref[perm].contiguous(), deg[perm].contiguous(), 16000,
                   lengths=torch.tensor(lens)[perm])
    assert torch.equal(_bits(dp), _bits(d)[perm])
    again = ops.estoi(ref, deg, 16000, lengths=lens)
    assert torch.equal(_bits(again), _bits(d))


def test_validation_errors():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 8000, device='cuda')
    with pytest.raises(ValueError):
        ops.estoi(x, x[:, :7999].contiguous())
    with pytest.raises(ValueError):
        quality.estoi(x[0], x[0, :7000])
    for bad in ([8000], [8000, 8001], [-1, 5], [1.5, 2.0], [[1, 2]]):
        with pytest.raises(ValueError):
            ops.estoi(x, x, lengths=bad)
    for sr in (3999, 48001, 16000.5, True):
        with pytest.raises(ValueError):
            quality.estoi(x, x, srate=sr)
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.estoi(x.cpu(), x.cpu())
    assert quality.estoi(x[0], x[0]).shape == (1,)


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


@pytest.mark.parametrize('flags,columns', [(['--estoi'], ['ESTOI']),
                                           (['--stoi', '--estoi'], ['STOI', 'ESTOI'])])
def test_eval_noisy_performance_estoi_column(sfx, efx, tmp_path, flags, columns):
    from scipy.io import wavfile
    cli = sfx['cli']
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    for name, c, n in zip(cli['names'], cli['clean'], cli['noisy']):
        wavfile.write(str(cdir / name), 16000, c.numpy())
        wavfile.write(str(ndir / name), 16000, n.numpy())
    log = tmp_path / 'eval.log'
    env = dict(os.environ)
    env['PATH'] = _fake_pesqmain(tmp_path, '2.500') + os.pathsep + env['PATH']
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable,
                        os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
                        '--clean_wavs', str(cdir), '--logfile', str(log)] + flags,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR ' + ' '.join(columns)
    assert [l.split()[0] for l in lines[1:]] == cli['names']
    want = {'STOI': cli['d'].tolist(), 'ESTOI': efx['cli_d'].tolist()}
    for k, line in enumerate(lines[1:]):
        f = line.split()
        assert len(f) == 6 + len(columns), line
        for col, v in zip(columns, f[6:]):
            assert len(v.split('.')[1]) == 4, line
            assert abs(float(v) - want[col][k]) <= 5e-5 + 1e-12, (line, col, want[col][k])
    for col in columns:
        assert 'mean {}: '.format(col) in p.stdout
    assert ('mean STOI: ' in p.stdout) == ('STOI' in columns)
    assert p.stdout.index('mean Covl: ') < p.stdout.index('mean ESTOI: ')
    assert 'Processed 3/3 wav' in p.stdout


def test_evaluate_adds_estoi_only_when_asked(tmp_path, monkeypatch):
    from segan_pytorch_amd import ops, quality
    from segan_pytorch_amd.models import SEGAN
    from segan_pytorch_amd.datasets import synthetic_pairs
    frows = load_golden('frows.pt')
    o = dict(frows['generate']['opts'])
    o.update(save_path=str(tmp_path), eval_workers=2)
    torch.manual_seed(3)
    m = SEGAN(SimpleNamespace(**o)).to('cuda')
    vc, vn = synthetic_pairs(2, 16384, 2)
    va = [[['v'] * 2, vc, vn, torch.zeros(2)]]
    monkeypatch.setenv('PATH', _fake_pesqmain(tmp_path, '3.250') + os.pathsep + os.environ['PATH'])
    base = {'ssnr', 'snr', 'pesq', 'csig', 'cbak', 'covl', 'wss', 'llr'}
    o['eval_stoi'] = True
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'stoi'}
    o.update(eval_stoi=False, eval_estoi=True)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'estoi'}
    assert len(ev['estoi']) == len(nev['estoi']) == 2
    c = ops.de_emphasize(vc.cuda().float().contiguous(), m.preemph)
    d = ops.de_emphasize(vn.cuda().float().contiguous(), m.preemph)
    want = quality.estoi(c, d).cpu().tolist()
    assert nev['estoi'] == want and all(np.isfinite(want))
    assert all(math.isnan(v) or -1 <= v <= 1 for v in ev['estoi'])
