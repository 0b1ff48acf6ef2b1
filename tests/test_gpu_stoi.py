"""STOI on the MI355X (ops.stoi / ops.stoi_stages, quality.stoi, SEGAN.evaluate with eval_stoi,
eval_noisy_performance.py --stoi) against the fp64 numpy oracle (scripts/stoi_oracle.py ->
tests/golden/stoi.pt, recipe scripts/make_golden_stoi.py)."""
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
from make_golden_stoi import case_signals  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def sfx():
    return load_golden('stoi.pt')


def _cuda(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda().unsqueeze(0) for a in arrs]


def _bits(t):
    return t.detach().cpu().view(torch.int64)


def _close_peak(got, want, tol):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert (got - want).abs().max().item() <= tol * want.abs().max().item()


@pytest.mark.parametrize('name', ['stage16k', 'stage8k'])
def test_stages_match_the_oracle(sfx, name):
    from segan_pytorch_amd import ops
    ref, deg, sr = case_signals(sfx, name)
    st = ops.stoi_stages(*_cuda(ref, deg), srate=sr)
    want = sfx['stages'][name]
    _close_peak(st['xr'][0].cpu(), want['xr'], 1e-12)
    _close_peak(st['yr'][0].cpu(), want['yr'], 1e-12)
    assert torch.equal(st['mask'][0].cpu(), want['mask'])
    M = int(st['count'][0])
    assert M == want['M']
    assert torch.equal(st['kept'][0, :M].cpu().long(), torch.nonzero(want['mask']).view(-1))
    Lc = (M - 1) * 128 + 256
    _close_peak(st['xs'][0, :Lc].cpu(), want['xs'], 1e-12)
    _close_peak(st['ys'][0, :Lc].cpu(), want['ys'], 1e-12)
    for k in ('X', 'Y'):
        got, w = st[k][0, :, :M - 1].cpu(), want[k]
        assert got.shape == w.shape
        rowmax = w.abs().max(dim=1, keepdim=True).values
        assert torch.all((got - w).abs() <= 1e-10 * rowmax), k
    rho = st['rho'][0, :M - 30].cpu()
    assert rho.shape == want['rho'].shape
    assert torch.equal(torch.isnan(rho), torch.isnan(want['rho']))
    assert (rho - want['rho']).nan_to_num().abs().max().item() <= 1e-7
    assert abs(float(st['d'][0]) - want['d']) <= 1e-8


# srate -> T with ceil(T p / q) = 257 outputs, one past the kernel's 256-output tile: tap table in
# LDS with p > q, in LDS with p < q, 9000 doubles read through L2 (p = 200), q = 24, identity
@pytest.mark.parametrize('srate,T', [(8000, 205), (16000, 410), (22050, 565), (48000, 1229),
                                     (10000, 257)])
def test_stage_1_is_bitwise_the_public_resampler_with_scipys_filter(srate, T):
    """STOI's resampling to 10 kHz runs through the kernel of ops.resample: xr / yr carry the bits
    of ops.resample(..., 10000, fp64 out, zeros 10, beta 5.0) wherever the two designer modes give
    the same taps, as they do at these rates.  Rows of length 0, 1 and T with junk past the
    length: the row start, the row end, the tile edge and the zero fill."""
    from segan_pytorch_amd import ops
    g = torch.Generator().manual_seed(srate)
    ref = torch.randn(3, T, generator=g).cuda()
    deg = torch.randn(3, T, generator=g).cuda()
    lens = [0, 1, T]
    st = ops.stoi_stages(ref, deg, srate, lengths=lens)
    assert st['dims'][0] == 257
    for key, x in (('xr', ref), ('yr', deg)):
        y, info = ops.resample(x, srate, 10000, lens, torch.float64, 10, 5.0)
        assert y.shape == st[key].shape == (3, 257)
        one = -(-10000 // srate)   # the samples one sample becomes
        assert info['lengths'].tolist() == [0, one, 257]
        assert torch.equal(_bits(st[key].contiguous()), _bits(y)), (srate, key)
        assert not y[0].any() and not y[1, one:].any() and y[1, :one].all() and y[2].all()


def test_every_fixture_case(sfx):
    from segan_pytorch_amd import ops
    for name in sfx['cases']:
        ref, deg, sr = case_signals(sfx, name)
        d = ops.stoi(*_cuda(ref, deg), srate=sr)
        assert d.dtype == torch.float64 and d.shape == (1,)
        got, want = float(d[0]), sfx['d'][name]
        if math.isnan(want):
            assert math.isnan(got), (name, got)
        else:
            assert abs(got - want) <= 1e-8, (name, got, want)


def test_identity_scaling_and_snr_order(sfx):
    from segan_pytorch_amd.quality import stoi
    ref, _, _ = case_signals(sfx, 'snr0')
    x = torch.from_numpy(ref).cuda()
    assert abs(float(stoi(x, x)[0]) - 1) <= 1e-12
    assert abs(float(stoi(x, x * 0.25)[0]) - 1) <= 1e-12
    names = ['snrm5', 'snr0', 'snr10', 'snr20']
    pairs = [case_signals(sfx, n)[:2] for n in names]
    d = stoi(torch.from_numpy(np.stack([p[0] for p in pairs])).cuda(),
             torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()).cpu()
    assert torch.all(d[1:] > d[:-1]), d


def _padded(sfx, names):
    sigs = [case_signals(sfx, n)[:2] for n in names]
    T = max(len(r) for r, _ in sigs)
    ref = np.zeros((len(sigs), T), np.float32)
    deg = np.full((len(sigs), T), 0.7, np.float32)   # junk past each row's length
    for i, (r, d) in enumerate(sigs):
        ref[i, :len(r)] = r
        deg[i, :len(d)] = d
    return sigs, torch.from_numpy(ref).cuda(), torch.from_numpy(deg).cuda(), [len(r) for r, _ in sigs]


def test_batch_with_lengths_is_bitwise_the_single_row_call(sfx):
    from segan_pytorch_amd import ops
    names = [n for n, rc in sfx['cases'].items() if rc['srate'] == 16000]
    assert {'short', 'silent', 'odd_len', 'stage16k', 'snr0'} <= set(names)
    sigs, ref, deg, lens = _padded(sfx, names)
    d = ops.stoi(ref, deg, 16000, lengths=lens)
    single = torch.cat([ops.stoi(*_cuda(r, g), srate=16000) for r, g in sigs])
    assert torch.equal(_bits(d), _bits(single))
    perm = list(reversed(range(len(names))))
    dp = ops.stoi(ref[perm].contiguous(), deg[perm].contiguous(), 16000,
                  lengths=torch.tensor(lens)[perm])
    assert torch.equal(_bits(dp), _bits(d)[perm])
    again = ops.stoi(ref, deg, 16000, lengths=lens)
    assert torch.equal(_bits(again), _bits(d))


def test_validation_errors():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 8000, device='cuda')
    with pytest.raises(ValueError):
        ops.stoi(x, x[:, :7999].contiguous())
    with pytest.raises(ValueError):
        quality.stoi(x[0], x[0, :7000])
    for bad in ([8000], [8000, 8001], [-1, 5], [1.5, 2.0], [[1, 2]]):
        with pytest.raises(ValueError):
            ops.stoi(x, x, lengths=bad)
    for sr in (3999, 48001, 16000.5, True):
        with pytest.raises(ValueError):
            quality.stoi(x, x, srate=sr)
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.stoi(x.cpu(), x.cpu())
    assert quality.stoi(x[0], x[0]).shape == (1,)


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_eval_noisy_performance_stoi_column(sfx, tmp_path):
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
                        '--clean_wavs', str(cdir), '--logfile', str(log), '--stoi'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR STOI'
    assert [l.split()[0] for l in lines[1:]] == cli['names']
    for line, want in zip(lines[1:], cli['d'].tolist()):
        f = line.split()
        assert len(f) == 7 and len(f[6].split('.')[1]) == 4, line
        assert abs(float(f[6]) - want) <= 5e-5 + 1e-12, (line, want)
    assert 'mean STOI: ' in p.stdout and 'Processed 3/3 wav' in p.stdout


def test_evaluate_adds_stoi_only_when_asked(tmp_path, monkeypatch):
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
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert 'stoi' not in ev and 'stoi' not in nev
    o['eval_stoi'] = True
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == {'ssnr', 'snr', 'pesq', 'csig', 'cbak', 'covl', 'wss', 'llr',
                                   'stoi'}
    assert len(ev['stoi']) == len(nev['stoi']) == 2
    c = ops.de_emphasize(vc.cuda().float().contiguous(), m.preemph)
    d = ops.de_emphasize(vn.cuda().float().contiguous(), m.preemph)
    want = quality.stoi(c, d).cpu().tolist()
    assert nev['stoi'] == want and all(np.isfinite(want))
    assert all(math.isnan(v) or -1 <= v <= 1 for v in ev['stoi'])
