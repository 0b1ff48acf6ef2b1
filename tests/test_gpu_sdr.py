"""The BSS-eval SDR on the MI355X (ops.sdr / sdr_stages / toeplitz_solve, quality.sdr,
SEGAN.evaluate, eval_noisy_performance.py) against the fp64 numpy oracle scripts/sdr_oracle.py and
its fixture tests/golden/sdr.pt.

Tolerances: the SDR 1e-8 dB (what SI-SDR is asserted at; the oracle's two solvers agree within
meta.solver_gap_db < 1e-10).  The correlations: every product of two fp32 values is exact in fp64
and a lag is the sum of at most L of them, so |r - r_oracle| <= L 2^-52 r[0] (sum |s[t] s[t+k]| <=
r[0]) and |d - d_oracle| <= L 2^-52 sqrt(r[0] sum x^2) (Cauchy-Schwarz).  St and Ee: 1e-9
relative.  The solver: n 9 2^-52 relative in the max norm for Toeplitz(0.5^k), whose condition
number is about 9.  Every signal has at most 3 spans of 4096 samples."""
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
import make_golden_sdr as GS  # noqa: E402
import sdr_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
SDR_ATOL = 1e-8
ENERGY_RTOL = 1e-9
SPAN = 4096
TAPS = (1, 2, 33, 512)


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


@pytest.fixture(scope='module')
def sfx():
    return load_golden('sdr.pt')


def _cuda(*arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda().unsqueeze(0) for a in arrs)


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


@pytest.mark.parametrize('taps', TAPS)
def test_fixture_cases_match_the_oracle(qfx, sfx, taps):
    from segan_pytorch_amd import ops, quality
    assert tuple(sfx['taps']) == TAPS and ops.SDR_SPAN == SPAN
    worst = 0.0
    for name, rc in sfx['cases'].items():
        assert rc['len'] <= 3 * SPAN
        ref, deg = GS.case_signals(qfx, name)
        want = sfx['results'][name][taps]['sdr']
        r, d = _cuda(ref, deg)
        got = (ops.sdr(r, d, taps=taps), quality.sdr(r[0], d[0], taps=taps),
               ops.sdr_stages(r, d, taps=taps)['sdr'])
        for g in got:
            assert g.shape == (1,) and g.dtype == torch.float64 and g.is_cuda
            worst = max(worst, abs(float(g) - want))
    print('SDR worst error at {} taps: {:.3g} dB'.format(taps, worst))
    assert worst <= SDR_ATOL
    if taps == 512:     # the default
        ref, deg = GS.case_signals(qfx, 'short')
        r, d = _cuda(ref, deg)
        assert torch.equal(_bits(ops.sdr(r, d)), _bits(ops.sdr(r, d, taps=512)))
        assert torch.equal(_bits(quality.sdr(r, d)), _bits(ops.sdr(r, d, taps=512)))


@pytest.mark.parametrize('taps', TAPS)
def test_stages_match_the_oracle(qfx, sfx, taps):
    from segan_pytorch_amd import ops
    worst = {'r': 0.0, 'd': 0.0, 'St': 0.0, 'Ee': 0.0}
    for name, rc in sfx['cases'].items():
        ref, deg = GS.case_signals(qfx, name)
        L = len(ref)
        want = sfx['results'][name][taps]
        st = ops.sdr_stages(*_cuda(ref, deg), taps=taps)
        assert st['r'].shape == st['d'].shape == st['c'].shape == (1, taps)
        assert st['order'].shape == (1,) and not st['order'].dtype.is_floating_point
        assert int(st['order']) == want['order'] == taps
        wr, wd = want['r'].numpy(), want['d'].numpy()
        xx = float(np.dot(deg.astype(np.float64), deg.astype(np.float64)))
        er = np.abs(st['r'][0].cpu().numpy() - wr).max() / (L * 2.0 ** -52 * wr[0])
        ed = np.abs(st['d'][0].cpu().numpy() - wd).max() / (L * 2.0 ** -52 * math.sqrt(wr[0] * xx))
        eS = abs(float(st['target_energy']) - want['target_energy']) / want['target_energy']
        eE = abs(float(st['error_energy']) - want['error_energy']) / want['error_energy']
        for k, v in (('r', er), ('d', ed), ('St', eS), ('Ee', eE)):
            worst[k] = max(worst[k], v)
    print('SDR stages at {} taps: r, d at {:.3g}, {:.3g} of their bounds; St, Ee within {:.3g}, '
          '{:.3g} relative'.format(taps, worst['r'], worst['d'], worst['St'], worst['Ee']))
    assert worst['r'] <= 1.0 and worst['d'] <= 1.0
    assert worst['St'] <= ENERGY_RTOL and worst['Ee'] <= ENERGY_RTOL


def test_ragged_batch_is_bitwise_the_single_row_call(qfx):
    from segan_pytorch_amd import ops
    taps, T = 33, 2 * SPAN + 17
    lens = [1, 20, SPAN, SPAN + 1, 2 * SPAN + 17]
    ref, deg = GS.case_signals(qfx, 'snr10')
    rng = np.random.default_rng(11)
    R = rng.standard_normal((len(lens), T)).astype(np.float32)     # garbage past each length
    D = rng.standard_normal((len(lens), T)).astype(np.float32)
    for i, L in enumerate(lens):
        R[i, :L] = ref[:L]
        D[i, :L] = deg[:L]
    R, D = torch.from_numpy(R).cuda(), torch.from_numpy(D).cuda()
    got = ops.sdr_stages(R, D, lengths=lens, taps=taps)
    again = ops.sdr_stages(R, D, lengths=torch.tensor(lens), taps=taps)
    assert got['sdr'].shape == (5,) and got['c'].shape == (5, taps)
    for k in got:
        assert torch.equal(_bits(got[k].double()), _bits(again[k].double())), k
    assert torch.equal(_bits(ops.sdr(R, D, lengths=lens, taps=taps)), _bits(got['sdr']))
    for i, L in enumerate(lens):
        single = ops.sdr_stages(*_cuda(ref[:L], deg[:L]), taps=taps)
        for k in got:
            assert torch.equal(_bits(single[k].double()), _bits(got[k][i:i + 1].double())), (L, k)
        want = O.sdr_stages(ref[:L], deg[:L], taps)
        assert int(got['order'][i]) == want['order'] == taps
        if L > 1:     # one sample: Ee is a rounding residue
            assert abs(float(got['sdr'][i]) - want['sdr']) <= SDR_ATOL, L
    # lags at and past a row's length are exactly zero
    assert not got['r'][1, 20:].any() and not got['d'][1, 20:].any() and got['r'][1, 19] != 0
    assert not got['r'][0, 1:].any()
    # rows without samples are NaN and leave the others alone
    z = ops.sdr(R, D, lengths=[0, 20, 0, SPAN + 1, 0], taps=taps)
    assert torch.isnan(z[[0, 2, 4]]).all()
    assert torch.equal(_bits(z[[1, 3]]), _bits(got['sdr'][[1, 3]]))


@pytest.mark.parametrize('taps', [1, 33, 512])
def test_special_values(qfx, taps):
    from segan_pytorch_amd import ops
    ref, deg = GS.case_signals(qfx, 'snr10')
    ref, deg = ref[:SPAN + 905], deg[:SPAN + 905]
    r, d = _cuda(ref, deg)
    half = (0.5 * r).contiguous()
    rows = torch.cat([r, r, torch.zeros_like(r), r])
    degs = torch.cat([r.clone(), half, d, torch.zeros_like(r)])
    st = ops.sdr_stages(rows, degs, taps=taps)
    out = st['sdr'].cpu()
    assert out[0] == math.inf and out[1] == math.inf
    assert torch.isnan(out[2]) and torch.isnan(out[3])
    c = st['c'].cpu()
    assert c[0, 0] == 1.0 and c[1, 0] == 0.5 and not c[:2, 1:].any()
    assert st['order'].tolist() == [taps, taps, 0, taps]
    assert st['error_energy'][:2].cpu().tolist() == [0.0, 0.0]
    assert torch.equal(_bits(st['d'][1]), _bits(0.5 * st['r'][1]))
    if taps == 1:
        got = float(ops.sdr(r, d, taps=1))
        assert abs(got - O.sdr_one_tap(ref, deg)) <= SDR_ATOL


@pytest.mark.parametrize('n', [1, 2, 64, 512])
def test_toeplitz_solve_matches_numpy(n):
    from segan_pytorch_amd import ops
    r = 0.5 ** np.arange(n)
    d = np.random.default_rng(n).standard_normal((3, n))
    A = r[np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])]
    want = np.linalg.solve(A, d.T).T
    c, order = ops.toeplitz_solve(torch.from_numpy(np.tile(r, (3, 1))).cuda(),
                                  torch.from_numpy(d).cuda())
    assert c.shape == (3, n) and c.dtype == torch.float64 and order.tolist() == [n] * 3
    err = np.abs(c.cpu().numpy() - want).max(axis=1) / np.abs(want).max(axis=1)
    print('toeplitz_solve n = {}: {:.3g} relative (bound {:.3g})'.format(n, err.max(),
                                                                        n * 9 * 2.0 ** -52))
    assert err.max() <= n * 9 * 2.0 ** -52
    c1, o1 = ops.toeplitz_solve(torch.from_numpy(r).cuda(), torch.from_numpy(d[1]).cuda())
    assert c1.shape == (n,) and torch.equal(_bits(c1), _bits(c[1])) and o1.tolist() == [n]


def test_toeplitz_solve_guard_stops_a_rank_two_system():
    from segan_pytorch_amd import ops
    r = np.cos(0.3 * np.arange(64))
    rows = torch.from_numpy(np.stack([r, np.zeros(64), 0.5 ** np.arange(64)])).cuda()
    c, order = ops.toeplitz_solve(rows, rows.clone())
    assert order.tolist() == [2, 0, 64]
    c = c.cpu().numpy()
    assert not c[0, 2:].any() and not c[1].any()
    A = r[np.abs(np.arange(64)[:, None] - np.arange(64)[None, :])]
    assert np.abs(A @ c[0] - r).max() <= 1e-12
    want, _ = O.levinson(r, r.copy())
    assert np.abs(c[0] - want).max() <= 1e-12
    assert c[2, 0] == 1.0 and np.abs(c[2, 1:]).max() <= 1e-15


def test_validation_errors():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.sdr, ops.sdr_stages):
        with pytest.raises(ValueError):
            fn(x, x[:, :4999].contiguous())
        with pytest.raises(TypeError):
            fn(x.double(), x.double())
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu(), x.cpu())
        for bad in (0, 513):
            with pytest.raises(ValueError, match='taps'):
                fn(x, x, taps=bad)
        for bad in ([5000], [5000, 5001], [-1, 5], [1.5, 2.0], [[1, 2]]):
            with pytest.raises(ValueError):
                fn(x, x, lengths=bad)
    with pytest.raises(ValueError):
        quality.sdr(x[0], x[0, :4000])
    for bad in (0, 513):
        with pytest.raises(ValueError, match='taps'):
            quality.sdr(x, x, taps=bad)
    assert quality.sdr(x[0], x[0], taps=8).shape == (1,)
    assert quality.sdr(x, x, lengths=[5000, 0], taps=8).shape == (2,)
    r = torch.ones(2, 8, device='cuda', dtype=torch.float64)
    with pytest.raises(TypeError):
        ops.toeplitz_solve(r.float(), r.float())
    with pytest.raises(ValueError):
        ops.toeplitz_solve(r, r[:, :7])
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.toeplitz_solve(r.cpu(), r.cpu())


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_eval_noisy_performance_sdr_column(qfx, tmp_path):
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
        L = min(c.numel(), n.numel())
        assert L <= 17003
        cf, nf = (torch.from_numpy(t.numpy()[:L].astype(np.float32) / 32768).cuda() for t in (c, n))
        want.append((float(quality.si_sdr(cf, nf)), float(quality.sdr(cf, nf))))
    log = tmp_path / 'eval.log'
    env = dict(os.environ)
    env['PATH'] = _fake_pesqmain(tmp_path, cli['pesq']) + os.pathsep + env['PATH']
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable,
                        os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
                        '--clean_wavs', str(cdir), '--logfile', str(log), '--sisdr', '--sdr'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR SISDR SDR'
    assert [l.split()[0] for l in lines[1:]] == cli['names']
    for line, (w_si, w_sdr) in zip(lines[1:], want):
        f = line.split()
        assert len(f) == 8, line
        assert f[6] == '{:.4f}'.format(w_si) and f[7] == '{:.4f}'.format(w_sdr), line
    out = p.stdout
    assert out.index('mean Covl: ') < out.index('mean SISDR: ') < out.index('mean SDR: ')
    mean = float(out[out.index('mean SDR: '):].split()[2])
    assert abs(mean - np.mean([w for _, w in want])) <= 1e-4
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
    assert not hasattr(SimpleNamespace(**o), 'eval_sdr')
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base
    o.update(eval_sdr=True)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'sdr'}
    for e in (ev, nev):
        assert len(e['sdr']) == 2 and np.isfinite(e['sdr']).all()
    o.update(eval_sdr=False, eval_sisdr=True)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'sisdr'}
