"""Speech-quality measures on the MI355X (ops.wss / ops.llr, quality.composite_eval,
SEGAN.evaluate, eval_noisy_performance.py) against the REAL reference's segan/utils.py
(scripts/make_golden_quality.py -> tests/golden/quality.pt)."""
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
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


def make_pair(fx, name):
    """The pair `name` rebuilt from the stored signals exactly as the fixture script makes it."""
    rc = fx['recipes'][name]
    clean = fx['signals'][rc['ref']].numpy()
    noise = fx['signals'][rc['noise']].numpy()
    deg = (clean + np.float32(fx['gains'][rc['gain']]) * noise).astype(np.float32)[:rc['len_deg']]
    ref = clean[:rc['len_ref']].copy()
    if 'zero_ref' in rc:
        a, b = rc['zero_ref']
        ref[a:b] = 0
    return ref, deg, rc.get('srate', 16000)


def _rows(arrs):
    return torch.from_numpy(np.stack(arrs)).cuda()


def _check_frames(got, want, wss):
    got, want = got.cpu(), want
    assert got.shape == want.shape
    if wss:
        assert torch.all((got - want).abs() <= 1e-6 * want.abs().clamp(min=1.0)), \
            (got - want).abs().max().item()
    else:
        fin = torch.isfinite(want)
        assert torch.equal(torch.isfinite(got), fin)
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        if fin.any():
            assert (got[fin] - want[fin]).abs().max().item() <= 1e-4


@pytest.mark.parametrize('srate', [16000, 8000])
def test_frame_measures_match_the_reference(qfx, srate):
    from segan_pytorch_amd import ops
    names = [n for n, rc in qfx['recipes'].items() if rc.get('srate', 16000) == srate
             and rc['len_ref'] == rc['len_deg']]
    pairs = [make_pair(qfx, n) for n in names]
    for T in sorted({len(p[0]) for p in pairs}):
        group = [(n, p) for n, p in zip(names, pairs) if len(p[0]) == T]
        ref = _rows([p[0] for _, p in group])
        deg = _rows([p[1] for _, p in group])
        w = ops.wss(ref, deg, srate)
        l = ops.llr(ref, deg, srate)
        assert w.dtype == torch.float64 and l.dtype == torch.float64
        for i, (n, _) in enumerate(group):
            _check_frames(w[i], qfx['results'][n]['wss'], True)
            _check_frames(l[i], qfx['results'][n]['llr'], False)
    assert len(names) >= (1 if srate == 8000 else 3)


def test_composite_eval_matches_the_reference(qfx):
    from segan_pytorch_amd.quality import composite_eval
    for name, res in qfx['results'].items():
        if 'composite' not in res:
            continue
        ref, deg, _ = make_pair(qfx, name)
        for s, want in res['composite'].items():
            r = composite_eval(torch.from_numpy(ref).cuda(), torch.from_numpy(deg).cuda(), pesq=s)
            got = torch.stack([r[k][0].cpu() for k in ('csig', 'cbak', 'covl', 'pesq', 'ssnr')])
            if name == 'short':
                assert torch.isnan(got).all(), got
                continue
            assert torch.equal(torch.isnan(got), torch.isnan(want)), (name, s, got, want)
            fin = torch.isfinite(want)
            assert (got[fin] - want[fin]).abs().max().item() <= 1e-4, (name, s, got, want)
    zr = qfx['results']['zero_run']['composite']['2.500']
    assert torch.isnan(zr[0]) and torch.isfinite(zr[1]) and torch.isnan(zr[2])


def test_frames_are_slice_invariant():
    """Frame f of a long row is computed from its own samples only: the frames from f0 on equal
    (bit for bit) those of the row sliced at f0 * hop."""
    from segan_pytorch_amd import ops
    g = torch.Generator().manual_seed(5)
    T = 120 * 16000
    x = torch.randn(T, generator=g) * torch.sin(torch.arange(T) * 1e-4).abs()
    y = x + 0.3 * torch.randn(T, generator=g)
    ref, deg = x.float().cuda().unsqueeze(0), y.float().cuda().unsqueeze(0)
    w, l = ops.wss(ref, deg), ops.llr(ref, deg)
    assert w.shape[1] == (T - 480) // 120
    for f0 in (1, 777, 9001, w.shape[1] - 3):
        s = f0 * 120
        ws = ops.wss(ref[:, s:].contiguous(), deg[:, s:].contiguous())
        ls = ops.llr(ref[:, s:].contiguous(), deg[:, s:].contiguous())
        assert torch.equal(ws, w[:, f0:f0 + ws.shape[1]])
        assert torch.equal(ls, l[:, f0:f0 + ls.shape[1]])


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_evaluate_returns_the_composite_keys(tmp_path, monkeypatch):
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
    for e in (ev, nev):
        assert set(e) == {'ssnr', 'snr', 'pesq', 'csig', 'cbak', 'covl', 'wss', 'llr'}
        assert all(len(v) == 2 for v in e.values())
        assert e['pesq'] == [3.25, 3.25]
        for k in ('csig', 'cbak', 'covl'):
            assert all(1.0 <= v <= 5.0 for v in e[k]), (k, e[k])
        assert all(v >= 0 for v in e['wss']) and all(np.isfinite(e['llr']))


def test_eval_noisy_performance_cli(qfx, tmp_path):
    from scipy.io import wavfile
    cli = qfx['cli']
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    for name, c, n in zip(cli['names'], cli['clean'], cli['noisy']):
        wavfile.write(str(cdir / name), 16000, c.numpy())
        wavfile.write(str(ndir / name), 16000, n.numpy())
    log = tmp_path / 'eval.log'
    env = dict(os.environ)
    env['PATH'] = _fake_pesqmain(tmp_path, cli['pesq']) + os.pathsep + env['PATH']
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable,
                        os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
                        '--clean_wavs', str(cdir), '--logfile', str(log)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    want = ['FILE CSIG CBAK COVL PESQ SSNR'] + [
        '{} '.format(name) + cli['format'].format(*row.tolist())
        for name, row in zip(cli['names'], cli['rows'])]
    assert log.read_text().splitlines() == want
    assert 'mean Covl: ' in p.stdout and 'Processed 3/3 wav' in p.stdout
