"""fwSNRseg, the cepstrum distance and SI-SDR on the MI355X (ops.fwsegsnr / cepstral_distance /
si_sdr, quality.*, SEGAN.evaluate, eval_noisy_performance.py) against the fp64 numpy oracle
scripts/measures_oracle.py and its fixture tests/golden/measures.pt.

Tolerances, each against the oracle: fwSNRseg 1e-6 relative (the project's WSS tolerance; the
fixture recipe asserts that no band difference or clip decision sits closer than that), SI-SDR
1e-8 dB (the STOI tests' absolute tolerance), CD max(100 x the oracle's own measured sensitivity to
summation order and precision, 1e-9) (make_golden_measures.cd_tolerance)."""
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
import make_golden_measures as GM  # noqa: E402
import measures_oracle as M  # noqa: E402

pytestmark = pytest.mark.gpu
FW_RTOL = 1e-6
SISDR_ATOL = 1e-8
SPAN = 4096
LENS = [600, 719, 720, 40000]


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


@pytest.fixture(scope='module')
def mfx():
    return load_golden('measures.pt')


def _cuda(*arrs):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda().unsqueeze(0) for a in arrs)


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _close_frames(got, want, rtol=0.0, atol=0.0, what=''):
    """NaN in the same places, finite values within rtol * |want| + atol; returns the worst error
    relative to that bound's scale."""
    got = got.detach().cpu().numpy()
    want = np.asarray(want, dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    if not fin.any():
        return 0.0
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= rtol * np.abs(want[fin]) + atol), (what, err.max())
    return float((err / np.abs(want[fin])).max() if rtol else err.max())


def _close(got, want, rtol=0.0, atol=0.0, what=''):
    return _close_frames(got.reshape(-1), np.array([want]), rtol, atol, what)


@pytest.mark.parametrize('srate', [16000, 8000])
def test_fixture_cases_match_the_oracle(qfx, mfx, srate):
    from segan_pytorch_amd import ops, quality
    names = [n for n, rc in mfx['cases'].items() if rc['srate'] == srate]
    assert len(names) >= (1 if srate == 8000 else 5)
    cd_tol = GM.cd_tolerance(mfx['meta'])
    worst = {'fw': 0.0, 'cd': 0.0, 'sisdr': 0.0}
    for n in names:
        ref, deg, sr = GM.case_signals(qfx, n)
        want = mfx['results'][n]
        r, d = _cuda(ref, deg)
        fw_f, fw_v = ops.fwsegsnr(r, d, sr)
        cd_f = ops.cepstral_distance(r, d, sr)
        nf = M.frame_count(len(ref), sr)
        assert fw_f.shape == cd_f.shape == (1, nf) and fw_v.shape == (1,)
        worst['fw'] = max(worst['fw'], _close_frames(fw_f[0], want['fw_frames'], rtol=FW_RTOL, what=n))
        worst['cd'] = max(worst['cd'], _close_frames(cd_f[0], want['cd_frames'], atol=cd_tol, what=n))
        _close(fw_v, want['fw'], rtol=FW_RTOL, what=n)
        _close(quality.fwsegsnr(r[0], d[0], sr), want['fw'], rtol=FW_RTOL, what=n)
        _close(quality.cepstral_distance(r, d, sr), want['cd'], atol=cd_tol, what=n)
        worst['sisdr'] = max(worst['sisdr'], _close(ops.si_sdr(r, d), want['sisdr'],
                                                    atol=SISDR_ATOL, what=n))
        _close(quality.si_sdr(r[0], d[0]), want['sisdr'], atol=SISDR_ATOL, what=n)
    print('measures worst error at {} Hz: fwSNRseg {:.3g} (relative), CD {:.3g}, SI-SDR {:.3g} dB'
          .format(srate, worst['fw'], worst['cd'], worst['sisdr']))


def test_silent_frames_are_nan_and_leave_the_means(qfx, mfx):
    from segan_pytorch_amd import ops, quality
    ref, deg, sr = GM.case_signals(qfx, 'zero_run')
    r, d = _cuda(ref, deg)
    fw_f, fw_v = ops.fwsegsnr(r, d, sr)
    cd_f = ops.cepstral_distance(r, d, sr)
    nan = torch.isnan(fw_f[0]).cpu()
    assert int(nan.sum()) == mfx['meta']['zero_run_nan_frames'] == 13
    assert torch.equal(nan, torch.isnan(cd_f[0]).cpu())
    assert nan.nonzero().flatten().tolist() == list(range(167, 180))   # frames within 20000:22000
    fin = fw_f[0][~nan.cuda()]
    assert abs(float(fw_v) - float(fin.mean())) <= 1e-12
    assert math.isfinite(float(quality.cepstral_distance(r, d, sr)))
    # silence in the processed signal alone
    assert torch.equal(torch.isnan(ops.fwsegsnr(d, r, sr)[0][0]).cpu(), nan)
    assert torch.equal(torch.isnan(ops.cepstral_distance(d, r, sr)[0]).cpu(), nan)
    # silence throughout: no finite frame, NaN values
    z = torch.zeros_like(r)
    f, v = ops.fwsegsnr(z, d, sr)
    assert torch.isnan(f).all() and torch.isnan(v).all()
    assert torch.isnan(quality.cepstral_distance(z, d, sr)).all()


@pytest.mark.parametrize('srate', [16000, 8000])
def test_identical_signals_are_35_dB_zero_distance_and_inf(qfx, srate):
    from segan_pytorch_amd import ops
    ref = GM.case_signals(qfx, 'snr10' if srate == 16000 else 'sr8k')[0][:9000]
    r, = _cuda(ref)
    f, v = ops.fwsegsnr(r, r.clone(), srate)
    assert f.numel() > 0 and torch.all(f == 35.0) and float(v) == 35.0
    assert torch.all(ops.cepstral_distance(r, r.clone(), srate) == 0.0)
    assert float(ops.si_sdr(r, r.clone())) == math.inf


@pytest.mark.parametrize('T', [599, 600, 719, 720])
def test_frame_count_edges(qfx, mfx, T):
    from segan_pytorch_amd import ops, quality
    ref, deg, sr = GM.case_signals(qfx, 'snr10')
    ref, deg = ref[1000:1000 + T], deg[1000:1000 + T]
    nf = {599: 0, 600: 1, 719: 1, 720: 2}[T]
    assert M.frame_count(T, sr) == nf
    r, d = _cuda(ref, deg)
    fw_f, fw_v = ops.fwsegsnr(r, d, sr)
    cd_f = ops.cepstral_distance(r, d, sr)
    assert fw_f.shape == cd_f.shape == (1, nf) and fw_f.dtype == cd_f.dtype == torch.float64
    cd_v = quality.cepstral_distance(r, d, sr)
    assert fw_v.shape == cd_v.shape == (1,) and cd_v.dtype == torch.float64
    if nf == 0:
        assert torch.isnan(fw_v).all() and torch.isnan(cd_v).all()
        assert torch.isnan(quality.fwsegsnr(r, d, sr)).all()
        return
    _close_frames(fw_f[0], M.fwsegsnr_frames(ref, deg, sr), rtol=FW_RTOL)
    _close_frames(cd_f[0], M.cd_frames(ref, deg, sr), atol=GM.cd_tolerance(mfx['meta']))
    _close(fw_v, M.fwsegsnr(ref, deg, sr), rtol=FW_RTOL)
    _close(cd_v, M.cepstral_distance(ref, deg, sr), atol=GM.cd_tolerance(mfx['meta']))


def _padded_batch(ref, deg, lens):
    """Rows ref[:L] / deg[:L] padded to max(lens) with non-zero garbage."""
    T = max(lens)
    R = np.full((len(lens), T), -0.3, np.float32)
    D = np.full((len(lens), T), 0.7, np.float32)
    rng = np.random.default_rng(9)
    R += rng.standard_normal(R.shape).astype(np.float32)
    for i, L in enumerate(lens):
        R[i, :L] = ref[:L]
        D[i, :L] = deg[:L]
    return torch.from_numpy(R).cuda(), torch.from_numpy(D).cuda()


def test_batch_with_lengths_is_bitwise_the_single_row_call(qfx):
    from segan_pytorch_amd import ops
    ref, deg, sr = GM.case_signals(qfx, 'snr10')
    R, D = _padded_batch(ref, deg, LENS)
    fw_f, fw_v = ops.fwsegsnr(R, D, sr, lengths=LENS)
    cd_f = ops.cepstral_distance(R, D, sr, lengths=LENS)
    sd = ops.si_sdr(R, D, lengths=LENS)
    assert fw_f.shape == cd_f.shape == (4, 329) and fw_v.shape == sd.shape == (4,)
    for i, L in enumerate(LENS):
        nf = M.frame_count(L, sr)
        r, d = _cuda(ref[:L], deg[:L])
        f1, v1 = ops.fwsegsnr(r, d, sr)
        assert f1.shape == (1, nf)
        assert torch.equal(_bits(fw_f[i, :nf]), _bits(f1[0])), L
        assert torch.equal(_bits(fw_v[i:i + 1]), _bits(v1)), L
        assert torch.equal(_bits(cd_f[i, :nf]), _bits(ops.cepstral_distance(r, d, sr)[0])), L
        assert torch.equal(_bits(sd[i:i + 1]), _bits(ops.si_sdr(r, d))), L
        assert torch.isnan(fw_f[i, nf:]).all() and torch.isnan(cd_f[i, nf:]).all(), L
        assert torch.isfinite(fw_f[i, :nf]).all() and torch.isfinite(cd_f[i, :nf]).all(), L
    # a LongTensor of lengths, rows permuted: every row keeps its bits
    perm = [2, 0, 3, 1]
    fp, vp = ops.fwsegsnr(R[perm].contiguous(), D[perm].contiguous(), sr,
                          lengths=torch.tensor(LENS)[perm])
    assert torch.equal(_bits(vp), _bits(fw_v)[perm])
    assert torch.equal(torch.isnan(fp).cpu(), torch.isnan(fw_f).cpu()[perm])


def test_si_sdr_lengths_spans_and_bits(qfx, mfx):
    from segan_pytorch_amd import ops
    ref, deg, _ = GM.case_signals(qfx, 'snr20')
    lens = [1, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN - 1, 2 * SPAN + 1, 40000]
    assert ops.SISDR_SPAN == SPAN
    R, D = _padded_batch(ref, deg, lens)
    got = ops.si_sdr(R, D, lengths=lens)
    assert got.shape == (len(lens),) and got.dtype == torch.float64
    assert torch.equal(_bits(ops.si_sdr(R, D, lengths=lens)), _bits(got))   # two calls, same bits
    worst = 0.0
    for i, L in enumerate(lens):
        single = ops.si_sdr(*_cuda(ref[:L], deg[:L]))
        assert torch.equal(_bits(single), _bits(got[i:i + 1])), L
        want = M.si_sdr(ref[:L], deg[:L])
        if L == 1:
            assert math.isnan(want) and torch.isnan(single).all()
        else:
            worst = max(worst, _close(single, want, atol=SISDR_ATOL, what=L))
    _close(got[-1:], mfx['results']['snr20']['sisdr'], atol=SISDR_ATOL)
    print('SI-SDR worst error over lengths {}: {:.3g} dB'.format(lens, worst))


def test_si_sdr_invariance_inf_and_nan(qfx):
    from segan_pytorch_amd import ops
    ref, deg, _ = GM.case_signals(qfx, 'snr10')
    ref, deg = ref[:9001], deg[:9001]
    r, d = _cuda(ref, deg)
    base = float(ops.si_sdr(r, d))
    for g, dc in ((0.25, 0.0), (-3.0, 0.0), (1.0, 0.4), (7.5, -0.2)):
        x = (np.float32(g) * deg + np.float32(dc)).astype(np.float32)
        got = float(ops.si_sdr(r, _cuda(x)[0]))
        assert abs(got - M.si_sdr(ref, x)) <= SISDR_ATOL, (g, dc)
        assert abs(got - base) <= 1e-4, (g, dc)      # x is rounded to fp32 again: 1e-7 relative
    rows = torch.cat([r, torch.zeros_like(r), torch.full_like(r, 0.25), r])
    degs = torch.cat([r, d, d, d])
    out = ops.si_sdr(rows, degs).cpu()
    assert out[0] == math.inf and torch.isnan(out[1]) and float(out[3]) == base
    assert torch.isnan(out[2])      # a constant clean row: no energy once the mean is removed


def test_validation_errors():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 8000, device='cuda')
    for fn in (ops.fwsegsnr, ops.cepstral_distance, ops.si_sdr):
        with pytest.raises(ValueError):
            fn(x, x[:, :7999].contiguous())
        for bad in ([8000], [8000, 8001], [0, 5], [-1, 5], [1.5, 2.0], [[1, 2]]):
            with pytest.raises(ValueError):
                fn(x, x, lengths=bad)
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu(), x.cpu())
    for fn in (quality.fwsegsnr, quality.cepstral_distance, quality.si_sdr):
        with pytest.raises(ValueError):
            fn(x[0], x[0, :7000])
        assert fn(x[0], x[0]).shape == (1,)
        assert fn(x, x, lengths=[8000, 700]).shape == (2,)
    for sr in (0, -8000, 16000.5, True):
        with pytest.raises(ValueError):
            quality.fwsegsnr(x, x, srate=sr)


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_eval_noisy_performance_columns(qfx, mfx, tmp_path):
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
                        '--clean_wavs', str(cdir), '--logfile', str(log), '--sisdr', '--cd',
                        '--fwsegsnr'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR FWSEGSNR CD SISDR'
    assert [l.split()[0] for l in lines[1:]] == cli['names']
    for k, (line, row) in enumerate(zip(lines[1:], cli['rows'])):
        f = line.split()
        assert len(f) == 9, line
        assert ' '.join(f[:6]) == '{} '.format(cli['names'][k]) + cli['format'].format(*row.tolist())
        for col, key, v in zip(('FWSEGSNR', 'CD', 'SISDR'), ('fw', 'cd', 'sisdr'), f[6:]):
            assert len(v.split('.')[1]) == 4, line
            assert abs(float(v) - float(mfx['cli'][key][k])) <= 5e-5 + 1e-9, (line, col)
    out = p.stdout
    assert out.index('mean Covl: ') < out.index('mean FWSEGSNR: ') < out.index('mean CD: ') < \
        out.index('mean SISDR: ')
    assert 'mean STOI' not in out and 'Processed 3/3 wav' in out


def test_evaluate_adds_the_keys_only_when_asked(tmp_path, monkeypatch):
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
    o.update(eval_fwsegsnr=True, eval_cd=True, eval_sisdr=True)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'fwsegsnr', 'cd', 'sisdr'}
    for e in (ev, nev):
        assert all(len(e[k]) == 2 and np.isfinite(e[k]).all() for k in ('fwsegsnr', 'cd', 'sisdr'))
        assert all(-10 <= v <= 35 for v in e['fwsegsnr']) and all(0 <= v <= 10 for v in e['cd'])
    o.update(eval_fwsegsnr=False, eval_cd=False)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | {'sisdr'}
