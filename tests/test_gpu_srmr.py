"""SRMR and the power-of-two fp64 FFT on the MI355X (ops.fft_pow2, ops.srmr / srmr_stages,
quality.srmr, SEGAN.evaluate, eval_noisy_performance.py) against numpy.fft and the fp64 numpy /
scipy oracle scripts/srmr_oracle.py with its fixture tests/golden/srmr.pt.

Tolerances.  The FFT: c log2(n) 2^-52 ||x||_2 in the max norm with c = 8, the textbook bound of
a radix-2 transform with accurate twiddles (each of the log2 n passes adds at most a few 2^-52 of
the values it combines, and the l2 norm bounds the max norm).  SRMR, Ebar and the envelope
energies: relative max(1e-12, 100 meta.oracle_gap), where oracle_gap is the difference between the
oracle in float64 and in numpy.longdouble (the gammatone recursions of the low channels have poles
at 0.985 and amplify rounding); it must stay below 1e-8.  BW and K* are compared exactly.  Every
signal has at most 12305 samples.

Measured on an MI355X: the FFT at most 0.061 of its bound (forward, n = 4096); SRMR 4.4e-13, Ebar
5.3e-12 and the envelope energies 5.1e-14 relative, against a tolerance of 1.5e-9."""
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
import make_golden_srmr as GS  # noqa: E402

pytestmark = pytest.mark.gpu
FFT_C = 8
WL = 4096
LENS = [0, 4095, 4096, 4097, 5120, 12305]


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


@pytest.fixture(scope='module')
def sfx():
    return load_golden('srmr.pt')


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _row(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().unsqueeze(0)


@pytest.mark.parametrize('lg', [1, 2, 5, 12, 13, 17])
def test_fft_pow2_matches_numpy(lg):
    from segan_pytorch_amd import ops
    assert ops.FFT_LDS_LOG2 == 12      # 12 and 13: the largest single-workgroup size and twice it
    n, rows = 1 << lg, 3 if lg < 17 else 2
    rng = np.random.default_rng(lg)
    x = rng.standard_normal((rows, n)) + 1j * rng.standard_normal((rows, n))
    xd = torch.from_numpy(x).cuda()
    bound = FFT_C * lg * 2.0 ** -52 * np.linalg.norm(x, axis=1)
    fwd = ops.fft_pow2(xd)
    inv = ops.fft_pow2(xd, inverse=True)
    back = ops.fft_pow2(fwd, inverse=True)
    assert fwd.shape == (rows, n) and fwd.dtype == torch.complex128 and fwd.is_cuda
    err = {'forward': np.abs(fwd.cpu().numpy() - np.fft.fft(x, axis=1)).max(axis=1) / bound,
           'inverse': np.abs(inv.cpu().numpy() - np.fft.ifft(x, axis=1)).max(axis=1) / bound,
           'round trip': np.abs(back.cpu().numpy() - x).max(axis=1) / bound}
    print('fft_pow2 n = 2^{}: '.format(lg) + ', '.join(
        '{} {:.3g}'.format(k, v.max()) for k, v in err.items()) + ' of the bound')
    for k, v in err.items():
        assert v.max() <= 1.0, (k, v)
    one = ops.fft_pow2(xd[1])
    assert one.shape == (n,) and torch.equal(torch.view_as_real(one).cpu(),
                                             torch.view_as_real(fwd[1]).cpu())


def test_fixture_cases_match_the_oracle(qfx, sfx):
    from segan_pytorch_amd import ops, quality
    meta = sfx['meta']
    tol = max(1e-12, 100 * meta['oracle_gap'])
    assert tol <= 1e-8
    worst = {'srmr': 0.0, 'energy': 0.0, 'envelope_energy': 0.0}
    for name, rc in sfx['cases'].items():
        assert rc['len'] <= 12305
        x = _row(GS.case_signal(qfx, name))
        want = sfx['results'][name]
        st = ops.srmr_stages(x)
        assert st['energy'].shape == (1, 23, 8) and st['envelope_energy'].shape == (1, 23)
        assert st['cfs'].shape == (23,) and st['srmr'].shape == (1,)
        assert st['srmr'].dtype == torch.float64 and st['srmr'].is_cuda
        assert not st['kstar'].dtype.is_floating_point
        assert torch.equal(st['cfs'].cpu(), want['cfs'])
        assert int(st['kstar']) == want['kstar'] and float(st['bw']) == want['bw'], name
        for got in (st['srmr'], ops.srmr(x), quality.srmr(x[0]), quality.srmr(x, 16000)):
            worst['srmr'] = max(worst['srmr'], abs(float(got) - want['srmr']) / want['srmr'])
        for k in ('energy', 'envelope_energy'):
            w = want[k].numpy()
            worst[k] = max(worst[k], float(np.max(np.abs(st[k][0].cpu().numpy() - w) / w)))
    print('SRMR worst relative errors: srmr {:.3g}, energy {:.3g}, envelope_energy {:.3g} '
          '(tolerance {:.3g})'.format(worst['srmr'], worst['energy'], worst['envelope_energy'],
                                      tol))
    for k, v in worst.items():
        assert v <= tol, (k, v)


def test_ragged_batch_is_bitwise_the_single_row_call_for_every_chunking(qfx):
    from segan_pytorch_amd import ops
    base = GS.case_signal(qfx, 'dry')
    T = len(base)
    assert T == LENS[-1] == 12305
    X = np.random.default_rng(5).standard_normal((len(LENS), T)).astype(np.float32)   # garbage
    for i, L in enumerate(LENS):
        X[i, :L] = base[:L]
    X = torch.from_numpy(X).cuda()
    got = ops.srmr_stages(X, lengths=LENS)
    per_row = 8 * (46 * 16384 + 184 * 9 + 23 + 234)     # segan_srmr_dims: bytes of one row
    for cap in (per_row + 100, 2 * per_row + 100, 4 * per_row + 100):      # 1, 2, 4 rows a call
        again = ops.srmr_stages(X, lengths=torch.tensor(LENS), ws_cap=cap)
        for k in got:
            assert torch.equal(_bits(got[k].double()), _bits(again[k].double())), (cap, k)
    with pytest.raises(ValueError, match='ws_cap'):
        ops.srmr(X, lengths=LENS, ws_cap=per_row - 8)
    for i, L in enumerate(LENS):
        if L == 0:
            continue
        single = ops.srmr_stages(_row(base[:L]))
        for k in got:
            if k != 'cfs':
                assert torch.equal(_bits(single[k].double()),
                                   _bits(got[k][i:i + 1].double())), (L, k)
    out = got['srmr'].cpu()
    assert torch.isnan(out[:2]).all() and torch.isfinite(out[2:]).all()
    assert got['kstar'][:2].tolist() == [0, 0] and torch.isnan(got['bw'][:2]).all()
    assert not got['energy'][:2].any()


def test_power_of_two_gain_gives_the_same_bits_and_silence_is_nan(qfx):
    from segan_pytorch_amd import ops
    x = _row(GS.case_signal(qfx, 'snr20'))
    rows = torch.cat([x, 0.25 * x, torch.zeros_like(x)])
    st = ops.srmr_stages(rows)
    assert torch.equal(_bits(st['srmr'][0]), _bits(st['srmr'][1]))
    assert torch.equal(_bits(st['energy'][0] * 0.0625), _bits(st['energy'][1]))
    assert torch.equal(_bits(st['bw'][0]), _bits(st['bw'][1]))
    assert math.isnan(float(st['srmr'][2])) and int(st['kstar'][2]) == 0
    assert math.isfinite(float(st['srmr'][0]))


def test_eight_kilohertz(qfx):
    import srmr_oracle as O
    from segan_pytorch_amd import ops, quality
    x = qfx['signals']['clean8'].numpy()[:6000]
    want = O.stages(x, 8000)
    ext = O.stages(x, 8000, dtype=np.longdouble)
    tol = max(1e-12, 100 * GS.rel_gap(want, ext))
    assert tol <= 1e-8
    st = ops.srmr_stages(_row(x), rate=8000)
    assert torch.equal(st['cfs'].cpu(), torch.from_numpy(want['cfs']))
    assert int(st['kstar']) == want['kstar'] and float(st['bw']) == want['bw']
    assert abs(float(st['srmr']) - want['srmr']) <= tol * want['srmr']
    assert float(quality.srmr(_row(x), srate=8000)) == float(st['srmr'])
    assert math.isnan(float(ops.srmr(_row(x[:2047]), rate=8000)))


def test_validation_errors():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.srmr, ops.srmr_stages):
        with pytest.raises(TypeError):
            fn(x.double())
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu())
        with pytest.raises(ValueError):
            fn(x[0])
        for bad in (44100, 0, 16000.5, True):
            with pytest.raises(ValueError, match='rate'):
                fn(x, rate=bad)
        for bad in ([5000], [5000, 5001], [-1, 5], [1.5, 2.0], [[1, 2]]):
            with pytest.raises(ValueError):
                fn(x, lengths=bad)
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.srmr(x.cpu())
    assert quality.srmr(x[0]).shape == (1,)
    assert quality.srmr(x, lengths=[5000, 0]).shape == (2,)
    z = torch.zeros(2, 8, device='cuda', dtype=torch.complex128)
    with pytest.raises(TypeError):
        ops.fft_pow2(z.to(torch.complex64))
    with pytest.raises(ValueError):
        ops.fft_pow2(z[:, :6])
    with pytest.raises(ValueError):
        ops.fft_pow2(z[:, :1])
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.fft_pow2(z.cpu())


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_eval_noisy_performance_srmr_column(qfx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import quality
    cli = qfx['cli']
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    want = []
    for name, c, n in zip(cli['names'], cli['clean'], cli['noisy']):
        wavfile.write(str(cdir / name), 16000, c.numpy())
        wavfile.write(str(ndir / name), 16000, n.numpy())
        assert WL <= n.numel() <= 17003
        nf = torch.from_numpy(n.numpy().astype(np.float32) / 32768).cuda()
        want.append(float(quality.srmr(nf)))
    log = tmp_path / 'eval.log'
    env = dict(os.environ)
    env['PATH'] = _fake_pesqmain(tmp_path, cli['pesq']) + os.pathsep + env['PATH']
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable,
                        os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
                        '--clean_wavs', str(cdir), '--logfile', str(log), '--srmr', '--sisdr'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR SISDR SRMR'
    assert [l.split()[0] for l in lines[1:]] == cli['names']
    for line, w in zip(lines[1:], want):
        f = line.split()
        assert len(f) == 8 and math.isfinite(w), line
        assert f[7] == '{:.4f}'.format(w), line
    out = p.stdout
    assert out.index('mean Covl: ') < out.index('mean SISDR: ') < out.index('mean SRMR: ')
    mean = float(out[out.index('mean SRMR: '):].split()[2])
    assert abs(mean - np.mean(want)) <= 1e-4
    assert 'Processed 3/3 wav' in out


def test_evaluate_adds_the_key_only_when_asked(tmp_path, monkeypatch):
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
    assert not hasattr(SimpleNamespace(**o), 'eval_srmr')
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base
    o.update(eval_srmr=True)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'srmr'}
    for e in (ev, nev):
        assert len(e['srmr']) == 2 and np.isfinite(e['srmr']).all()
    o.update(eval_srmr=False, eval_sdr=True)
    ev = m.evaluate(SimpleNamespace(**o), va, 1, device='cuda')
    assert set(ev) == base | {'sdr'}


def test_clean_prints_the_srmr_of_each_file_only_when_asked(tmp_path, capsys):
    import json
    from scipy.io import wavfile
    import clean
    from segan_pytorch_amd import quality
    from segan_pytorch_amd.models import SEGAN
    o = dict(load_golden('frows.pt')['generate']['opts'])
    o.update(save_path=str(tmp_path))
    torch.manual_seed(3)
    m = SEGAN(SimpleNamespace(**o))
    ckpt, cfg = str(tmp_path / 'g.ckpt'), str(tmp_path / 'train.opts')
    torch.save({'state_dict': m.G.state_dict()}, ckpt)
    with open(cfg, 'w') as f:
        json.dump(o, f)
    wav_dir, out_dir = tmp_path / 'noisy', tmp_path / 'enh'
    wav_dir.mkdir()
    out_dir.mkdir()
    rng = np.random.default_rng(0)
    for name in ('a.wav', 'b.wav'):
        wavfile.write(str(wav_dir / name), 16000,
                      (rng.standard_normal(9000) * 3000).astype(np.int16))
    args = dict(g_pretrained_ckpt=ckpt, cfg_file=cfg, test_files=[str(wav_dir)], h5=False,
                seed=111, synthesis_path=str(out_dir), cuda=True, soundfile=False)
    clean.main(SimpleNamespace(**args))
    assert 'SRMR' not in capsys.readouterr().out
    clean.main(SimpleNamespace(srmr=True, **args))
    out = capsys.readouterr().out
    want = []
    for name in ('a.wav', 'b.wav'):
        rate, enh = wavfile.read(str(out_dir / name))
        assert rate == 16000 and enh.dtype == np.float32 and len(enh) == 9000
        want.append(float(quality.srmr(torch.from_numpy(enh).cuda())))
        assert math.isfinite(want[-1])
        assert 'SRMR {}: {:.4f}'.format(out_dir / name, want[-1]) in out
    assert abs(float(out[out.index('mean SRMR: '):].split()[2]) - np.mean(want)) <= 1e-4
