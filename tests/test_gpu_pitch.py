"""The pitch tracker and the F0 / voicing measures on the MI355X (ops.pitch / pitch_stages /
f0_eval, quality.pitch / f0_eval, SEGAN.evaluate, eval_noisy_performance.py --f0) against the numpy
oracle scripts/pitch_oracle.py and its fixture tests/golden/pitch.pt.

Decisions.  No frame of the fixture has a decision margin below 1e-7 (the smallest is 3.3e-5),
seven orders of magnitude above the rounding of d', so `lag` and the voiced flag are compared
exactly on every frame, with no exemption.

Tolerances: 100 x the movement of the oracle between float64 and numpy.longdouble, per quantity,
as scripts/make_golden_pitch.py measured it (meta.gaps): d' and ap relative to the cancellation
scale (E(0) + E(tau)) tau / c(tau) of the element (ap: the largest over the lag range), 5.3e-13
and 3.4e-13; f0 relative, 4.7e-14; f0_mae and f0_kld relative to max(|value|, 1), 2.3e-13 and
1.8e-12; vuv_acc and voiced, ratios of two integers, exactly.

Measured on an MI355X (each test prints its figures): d', ap and f0 at distance 0 from the oracle
on every frame of every case, 8 kHz included (the tracker is bit-equal, as the whisper stage was);
f0_mae at most 1.2e-15, f0_kld at distance 0.  The tolerances stay as asserted."""
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
import make_golden_pitch as GP  # noqa: E402
import pitch_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def pfx():
    return load_golden('pitch.pt')


def _tol(pfx, k):
    return 100 * pfx['meta']['gaps'][k]


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _ragged(pfx):
    """the rows glide[:L] of the fixture's lengths in one batch, garbage past each length"""
    base, lens = pfx['signals']['glide'].numpy(), pfx['lengths']
    X = np.random.default_rng(5).standard_normal((len(lens), len(base))).astype(np.float32)
    for i, L in enumerate(lens):
        X[i, :L] = base[:L]
    return _cuda(X), lens


def _check_track(pfx, got, i, want, worst, srate=16000):
    """row i of a dict of ops.pitch_stages against a fixture entry; updates the worst figures"""
    nf = len(want['lag'])
    assert int(got['nframes'][i]) == nf
    lag, f0, ap = (got[k][i].cpu().numpy() for k in ('lag', 'f0', 'ap'))
    assert np.array_equal(lag[:nf], want['lag'].numpy())
    assert (lag[nf:] == -1).all() and (f0[nf:] == 0).all() and np.isnan(ap[nf:]).all()
    w = want['f0'].numpy()
    v = w > 0
    assert np.array_equal(f0[:nf] > 0, v)
    if v.any():
        worst['f0'] = max(worst['f0'], float(np.max(np.abs(f0[:nf] - w)[v] / w[v])))
    s = want['ap_scale'].numpy()
    da = np.abs(ap[:nf] - want['ap'].numpy())
    assert not da[s == 0].any()
    if (s > 0).any():
        worst['ap'] = max(worst['ap'], float(np.max(da[s > 0] / s[s > 0])))
    if 'cmnd' in want and 'cmnd' in got:
        c = got['cmnd'][i].cpu().numpy()
        assert np.isnan(c[nf:]).all()
        sc, dc = want['scale'].numpy(), np.abs(c[:nf] - want['cmnd'].numpy())
        assert not dc[sc == 0].any()           # the constant 1 where c(tau) is not positive
        if (sc > 0).any():
            worst['cmnd'] = max(worst['cmnd'], float(np.max(dc[sc > 0] / sc[sc > 0])))


def _assert_worst(pfx, worst, what):
    print('{}: worst errors '.format(what) + ', '.join(
        '{} {:.3g} (tolerance {:.3g})'.format(k, v, _tol(pfx, k)) for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= _tol(pfx, k), (k, v)


def test_ragged_batch_matches_the_oracle_on_every_frame(pfx):
    from segan_pytorch_amd import ops
    X, lens = _ragged(pfx)
    got = ops.pitch_stages(X, lengths=lens)
    assert got['f0'].shape == got['lag'].shape == got['ap'].shape == (8, 197)
    assert got['cmnd'].shape == (8, 197, 268) and got['lag'].dtype == torch.int32
    assert got['f0'].dtype == got['ap'].dtype == got['cmnd'].dtype == torch.float64
    assert got['nframes'].tolist() == [0, 0, 0, 0, 1, 2, 42, 197]
    worst = {'f0': 0.0, 'ap': 0.0, 'cmnd': 0.0}
    for i, L in enumerate(lens):
        _check_track(pfx, got, i, pfx['ragged'][L], worst)
    assert int((got['lag'][7] > 0).sum()) > 150
    _assert_worst(pfx, worst, 'ragged batch')


def test_a_batched_row_is_bitwise_its_own_call_for_every_chunking(pfx):
    from segan_pytorch_amd import ops
    X, lens = _ragged(pfx)
    got = ops.pitch_stages(X, lengths=lens)
    per_row = 8 * 201 * 2 * 268
    again = ops.pitch_stages(X, lengths=torch.tensor(lens), ws_cap=3 * per_row + 100)
    for k in got:
        assert torch.equal(_bits(got[k].double()), _bits(again[k].double())), k
    with pytest.raises(ValueError, match='ws_cap'):
        ops.pitch(X, lengths=lens, ws_cap=per_row - 8)
    base = pfx['signals']['glide'].numpy()
    for i, L in enumerate(lens):
        if L == 0:
            continue
        one = ops.pitch_stages(_cuda(base[:L]).unsqueeze(0))
        nf = int(one['nframes'][0])
        assert nf == int(got['nframes'][i]) == one['f0'].shape[1]
        for k in ('f0', 'ap', 'cmnd'):
            assert torch.equal(_bits(one[k][0]), _bits(got[k][i, :nf])), (L, k)
        assert torch.equal(one['lag'][0].cpu(), got['lag'][i, :nf].cpu())
    f0, lag, ap, nfr = ops.pitch(X, lengths=lens)
    assert torch.equal(_bits(f0), _bits(got['f0'])) and torch.equal(lag.cpu(), got['lag'].cpu())
    assert torch.equal(nfr.cpu(), got['nframes'].cpu())


def test_power_of_two_gains_silence_and_a_constant(pfx):
    from segan_pytorch_amd import ops, quality
    x = pfx['signals']['speech'][:8000].cuda().unsqueeze(0)
    rows = torch.cat([x, x * 2.0 ** -9, x * 2.0 ** 6, torch.zeros_like(x),
                      torch.full_like(x, 0.25)])
    f0, lag, ap, nfr = ops.pitch(rows)
    assert nfr.tolist() == [92] * 5 and int((lag[0] > 0).sum()) > 40
    for i in (1, 2):
        assert torch.equal(lag[i].cpu(), lag[0].cpu())
        assert torch.equal(_bits(f0[i]), _bits(f0[0])) and torch.equal(_bits(ap[i]), _bits(ap[0]))
    for i in (3, 4):
        assert not lag[i].any() and not f0[i].any() and (ap[i] == 1.0).all()
    qf0, voiced, qap = quality.pitch(rows)
    assert voiced.dtype == torch.bool and torch.equal(voiced.cpu(), (lag > 0).cpu())
    assert torch.equal(_bits(qf0), _bits(f0))
    assert quality.pitch(rows[0])[0].shape == (1, 92)


@pytest.mark.parametrize('theta', [0.15, 0.1, 0.3])
def test_threshold_changes_decisions_as_the_oracle_says(pfx, theta):
    from segan_pytorch_amd import ops
    x = pfx['signals']['speech'].cuda().unsqueeze(0)
    f0, lag, ap, nfr = ops.pitch(x, threshold=theta)
    worst = {'f0': 0.0, 'ap': 0.0}
    got = {'f0': f0, 'lag': lag, 'ap': ap, 'nframes': nfr}
    _check_track(pfx, got, 0, pfx['tracks']['speech@{}'.format(theta)], worst)
    _assert_worst(pfx, worst, 'theta {}'.format(theta))
    if theta != 0.15:
        other = pfx['tracks']['speech@0.15']['lag']
        assert not torch.equal(lag[0].cpu(), other)


def test_eight_kilohertz(pfx):
    from segan_pytorch_amd import ops
    x = pfx['signals']['speech8'].numpy()
    X = np.zeros((2, GP.N8), np.float32)
    X[0], X[1, :GP.N8_SHORT] = x, x[:GP.N8_SHORT]
    got = ops.pitch_stages(_cuda(X), lengths=[GP.N8, GP.N8_SHORT], srate=8000)
    assert got['cmnd'].shape == (2, 142, 135) and got['nframes'].tolist() == [142, 17]
    worst = {'f0': 0.0, 'ap': 0.0, 'cmnd': 0.0}
    _check_track(pfx, got, 0, pfx['tracks']['speech8'], worst, 8000)
    _check_track(pfx, got, 1, pfx['tracks']['speech8_short'], worst, 8000)
    assert int((got['lag'][0] > 0).sum()) == 90
    _assert_worst(pfx, worst, '8 kHz')


def _check_eval(pfx, got, want, worst):
    for k in ('vuv_acc', 'voiced'):
        g, w = float(got[k]), float(want[k])
        assert g == w or (math.isnan(g) and math.isnan(w)), (k, g, w)
    for k in ('f0_mae', 'f0_kld'):
        g, w = float(got[k]), float(want[k])
        assert math.isnan(g) == math.isnan(w), (k, g, w)
        if not math.isnan(w):
            worst[k] = max(worst[k], abs(g - w) / max(abs(w), 1.0))


def test_f0_eval_of_noisy_pairs_matches_the_oracle(pfx):
    from segan_pytorch_amd import ops, quality
    sig = {k: v.numpy() for k, v in pfx['signals'].items()}
    deg = GP.processed(sig, pfx['gains'])
    names = list(deg)
    assert names == ['snr20', 'snr10', 'snr5', 'noise']
    ref = _cuda(np.stack([sig['speech']] * len(names)))
    dg = _cuda(np.stack([deg[n] for n in names]))
    f0, lag, ap, nfr = ops.pitch(dg)
    worst = {'f0': 0.0, 'ap': 0.0}
    for i, n in enumerate(names):
        _check_track(pfx, {'f0': f0, 'lag': lag, 'ap': ap, 'nframes': nfr}, i, pfx['tracks'][n],
                     worst)
    _assert_worst(pfx, worst, 'noisy tracks')
    got = quality.f0_eval(ref, dg)
    assert set(got) == {'f0_mae', 'vuv_acc', 'f0_kld', 'voiced'}
    worst = {'f0_mae': 0.0, 'f0_kld': 0.0}
    for i, n in enumerate(names):
        for v in got.values():
            assert v.shape == (4,) and v.dtype == torch.float64 and v.is_cuda
        _check_eval(pfx, {k: v[i] for k, v in got.items()}, pfx['evals'][n], worst)
    one = quality.f0_eval(ref[1], dg[1], 16000)
    for k in got:
        assert torch.equal(_bits(one[k]), _bits(got[k][1:2])), k
    # per-row lengths: each row is the oracle's result on the truncated pair
    lens = [16384, 4001, 700, 0]
    cut = quality.f0_eval(ref, dg[[1, 1, 1, 1]], lengths=lens)
    for i, L in enumerate(lens):
        want = O.evaluate(sig['speech'][:L], deg['snr10'][:L])
        _check_eval(pfx, {k: v[i] for k, v in cut.items()}, want, worst)
    assert all(math.isnan(float(v[3])) for v in cut.values())
    _assert_worst(pfx, worst, 'f0_eval')


def test_f0_eval_nan_rules_and_long_gaps_on_given_contours(pfx):
    from segan_pytorch_amd import ops
    rng = np.random.default_rng(11)
    F = 300

    def contour_pair(voiced_r, voiced_d):
        fr = np.where(voiced_r, 16000.0 / rng.uniform(40, 266, F), 0.0)
        fd = np.where(voiced_d, fr * rng.uniform(0.9, 1.1, F) + (fr == 0) * 150.0, 0.0)
        return fr, voiced_r.astype(np.int32) * 100, fd, voiced_d.astype(np.int32) * 90

    idx = np.arange(F)
    none = np.zeros(F, bool)
    cases = [
        contour_pair(rng.random(F) < 0.5, rng.random(F) < 0.5),
        contour_pair((idx == 3) | (idx == 250), (idx > 100) & (idx < 180)),   # gaps over chunks
        contour_pair(idx == 299, idx == 0),
        contour_pair(idx % 64 == 63, idx % 64 == 0),
        contour_pair(none, rng.random(F) < 0.5),                              # no voiced ref
        contour_pair(rng.random(F) < 0.5, none),                              # no voiced deg
        contour_pair(none, none),
    ]
    # a constant processed contour over two frames: its mean is exact, so sigma_p is exactly 0
    c = np.where(idx % 7 == 0, 100.0, 0.0)
    cases.append((16000.0 / rng.uniform(40, 266, F), np.full(F, 100, np.int32), c,
                  (c > 0).astype(np.int32)))
    nframes = [F, F, F, 130, F, F, F, 2, 1, 0, 2, 65]
    while len(cases) < len(nframes):
        cases.append(cases[0])
    fr, lr, fd, ld = (_cuda(np.stack([c[j] for c in cases])) for j in range(4))
    out = ops.f0_eval(fr, lr, fd, ld, _cuda(np.asarray(nframes, np.int32)))
    assert out.shape == (len(cases), 4) and out.dtype == torch.float64
    out = out.cpu().numpy()
    worst = {'f0_mae': 0.0, 'f0_kld': 0.0}
    for i, (c, n) in enumerate(zip(cases, nframes)):
        want = O.f0_eval(c[0][:n], c[1][:n], c[2][:n], c[3][:n])
        _check_eval(pfx, dict(zip(('f0_mae', 'vuv_acc', 'f0_kld', 'voiced'), out[i])), want, worst)
    assert np.isfinite(out[:4]).all()
    assert np.isnan(out[4:7, 0]).all() and np.isnan(out[4:7, 2]).all()
    assert np.isfinite(out[4:7, 1]).all() and (out[4, 3], out[6, 1]) == (0.0, 1.0)
    assert math.isfinite(out[7, 0]) and math.isnan(out[7, 2])                 # sigma_p = 0
    assert math.isfinite(out[8, 1]) and math.isnan(out[8, 2])                 # one frame
    assert np.isnan(out[9]).all()                                             # no frame
    full = ops.f0_eval(fr, lr, fd, ld)
    assert np.array_equal(full.cpu().numpy()[:3], out[:3])
    _assert_worst(pfx, worst, 'given contours')


def test_validation_errors():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.pitch, ops.pitch_stages):
        with pytest.raises(TypeError):
            fn(x.double())
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu())
        with pytest.raises(ValueError, match='srate'):
            fn(x, srate=44100)
        with pytest.raises(ValueError, match='threshold'):
            fn(x, threshold=0.0)
        with pytest.raises(ValueError, match='lengths'):
            fn(x, lengths=[5000, 5001])
    with pytest.raises(ValueError, match='differ in shape'):
        quality.f0_eval(x, x[:, :4000])
    with pytest.raises(RuntimeError, match='MI355X'):
        quality.f0_eval(x.cpu(), x.cpu())
    short = quality.f0_eval(x[:, :600], x[:, :600])       # no frame: every measure is NaN
    assert all(torch.isnan(v).all() and v.shape == (2,) for v in short.values())
    f0, voiced, ap = quality.pitch(x[:, :600])
    assert f0.shape == voiced.shape == ap.shape == (2, 0)


def _fake_pesqmain(tmp_path, score):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t{}"\n'
                   .format(score))
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_eval_noisy_performance_f0_columns(pfx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import quality
    sig = {k: v.numpy() for k, v in pfx['signals'].items()}
    deg = GP.processed(sig, pfx['gains'])
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    names, want = ['a.wav', 'b.wav', 'c.wav'], []
    for name, d in zip(names, (deg['snr20'][:9000], deg['snr10'][:12000], deg['noise'][:8000])):
        c = sig['speech'][:len(d)]
        wavfile.write(str(cdir / name), 16000, c)
        wavfile.write(str(ndir / name), 16000, d)
        r = quality.f0_eval(_cuda(c), _cuda(d))
        want.append([float(r[k]) for k in ('f0_mae', 'vuv_acc', 'f0_kld')])
    assert math.isnan(want[2][0]) and math.isfinite(want[2][1]) and math.isfinite(want[0][0])
    log = tmp_path / 'eval.log'
    env = dict(os.environ)
    env['PATH'] = _fake_pesqmain(tmp_path, '2.500') + os.pathsep + env['PATH']
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable,
                        os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
                        '--clean_wavs', str(cdir), '--logfile', str(log), '--f0', '--sisdr'],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR SISDR F0MAE VUV F0KLD'
    assert [l.split()[0] for l in lines[1:]] == names
    for line, w in zip(lines[1:], want):
        f = line.split()
        assert len(f) == 10 and f[7:] == ['{:.4f}'.format(v) for v in w], line
    out = p.stdout
    assert out.index('mean SISDR: ') < out.index('mean F0MAE: ') < out.index('mean VUV: ') < (
        out.index('mean F0KLD: '))
    mae = out[out.index('mean F0MAE: '):].split('\n')[0]
    assert abs(float(mae.split()[2]) - np.mean([want[0][0], want[1][0]])) <= 1e-9
    assert '(1 NaN of 3 files)' in mae
    vuv = out[out.index('mean VUV: '):].split('\n')[0]
    assert '(0 NaN of 3 files)' in vuv
    assert abs(float(vuv.split()[2]) - np.mean([w[1] for w in want])) <= 1e-9


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
    f0k = {'f0_mae', 'vuv_acc', 'f0_kld'}
    assert not hasattr(SimpleNamespace(**o), 'eval_f0')
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base
    o.update(eval_f0=True)
    ev, nev = m.evaluate(SimpleNamespace(**o), va, 1, do_noisy=True, device='cuda')
    assert set(ev) == set(nev) == base | f0k
    for e in (ev, nev):
        assert all(len(e[k]) == 2 for k in f0k)
        assert np.isfinite(e['vuv_acc']).all() and (0 <= np.asarray(e['vuv_acc'])).all()
    o.update(eval_f0=False, eval_srmr=True)
    ev = m.evaluate(SimpleNamespace(**o), va, 1, device='cuda')
    assert set(ev) == base | {'srmr'}
