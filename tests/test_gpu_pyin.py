"""The Viterbi-smoothed pitch tracker on the MI355X (ops.pyin / pyin_stages, tracker='pyin' in
quality.pitch / f0_eval and eval_noisy_performance.py --f0_tracker) against the numpy oracle
scripts/pyin_oracle.py fed with the library's own tables.

Device and oracle perform the same IEEE operations in the same order, so nothing here has a
tolerance: the frame count, `state` and `lag` are compared on every frame of every row with no frame
exempted, and f0, vprob, bv and the last frame's delta bit for bit.  The rows are those of
scripts/make_golden_pyin.py (the fixture stores, for each, how far float64 and long double move
apart, should a value ever have to be compared at a distance; none has).  Only f0_eval's measures
keep the tolerances of tests/test_gpu_pitch.py, 100 x the float64 to long-double movement of
tests/golden/pitch.pt: they pass through log and exp."""
import math
import os
import stat
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_pyin as GP  # noqa: E402
import pitch_oracle as P  # noqa: E402
import pyin_oracle as Y  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def yfx():
    return load_golden('pyin.pt')


@pytest.fixture(scope='module')
def rows(yfx):
    return GP.rows({k: v.numpy() for k, v in yfx['signals'].items()})


@pytest.fixture(scope='module')
def oracle(rows):
    """every row's contour by the oracle on the library's tables, computed once"""
    from segan_pytorch_amd import ops
    tabs = {s: ops.pyin_tables(s) for s in (16000, 8000)}
    return {name: Y.track(x, srate, tabs=tabs[srate]) for name, (x, srate) in rows.items()}


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _check_row(got, i, want, name):
    """row i of a dict of ops.pyin_stages against the oracle's dict: equal on every frame"""
    nf = len(want['lag'])
    assert int(got['nframes'][i]) == nf, name
    st, lag = got['state'][i].cpu().numpy(), got['lag'][i].cpu().numpy()
    f0, vp = got['f0'][i].cpu().numpy(), got['vprob'][i].cpu().numpy()
    bv, dl = got['bv'][i].cpu().numpy(), got['delta'][i].cpu().numpy()
    assert np.array_equal(st[:nf], want['state']), (name, np.nonzero(st[:nf] != want['state'])[0])
    assert np.array_equal(lag[:nf], want['lag']), name
    assert (st[nf:] == -1).all() and (lag[nf:] == -1).all() and (f0[nf:] == 0).all(), name
    assert np.isnan(vp[nf:]).all() and np.isnan(bv[nf:]).all(), name
    worst = {k: float(np.max(np.abs(g - w))) if w.size else 0.0 for k, g, w in (
        ('f0', f0[:nf], want['f0']), ('vprob', vp[:nf], want['vprob']),
        ('bv', bv[:nf], want['bv']))}
    print('{}: frames {} largest distance from the oracle {}'.format(name, nf, worst))
    assert _same_bits(f0[:nf], want['f0']), name
    assert _same_bits(vp[:nf], want['vprob']), name
    assert _same_bits(bv[:nf], want['bv']), name
    if nf:
        assert _same_bits(dl, want['delta']), (name, float(np.max(np.abs(dl - want['delta']))))
    else:
        assert np.isnan(dl).all(), name


def test_every_row_equals_the_oracle_on_every_frame(rows, oracle):
    from segan_pytorch_amd import ops
    assert [len(rows['tone[:{}]'.format(L)][0]) for L in (666, 667, 747, 1707, 8000)] == [
        666, 667, 747, 1707, 8000]
    assert set(rows) >= {'tone8', 'zero', 'lead', 'tone*2^-10', 'gated5', 'octave'}
    for name, (x, srate) in rows.items():
        got = ops.pyin_stages(_cuda(x).unsqueeze(0), srate=srate)
        nf = P.n_frames(len(x), srate)
        assert got['f0'].shape == got['lag'].shape == got['vprob'].shape == (1, nf)
        assert got['state'].shape == (1, nf) and got['bv'].shape == (1, nf, 165)
        assert got['delta'].shape == (1, 330) and got['state'].dtype == got['lag'].dtype == torch.int32
        assert got['f0'].dtype == got['vprob'].dtype == got['bv'].dtype == torch.float64
        _check_row(got, 0, oracle[name], name)
        f0, lag, vp, nfr = ops.pyin(_cuda(x).unsqueeze(0), srate=srate)
        assert torch.equal(_bits(f0), _bits(got['f0'])) and torch.equal(lag, got['lag'])
        assert torch.equal(_bits(vp), _bits(got['vprob'])) and torch.equal(nfr, got['nframes'])
    assert oracle['tone[:1707]']['lag'].all() and len(oracle['tone[:1707]']['lag']) == 14
    g = oracle['gated5']
    assert 0 < int((g['lag'] > 0).sum()) < len(g['lag'])
    # a power of two changes no bit; the leading zeros decode unvoiced
    for k in ('f0', 'vprob', 'delta', 'bv'):
        assert _same_bits(oracle['tone*2^-10'][k], oracle['tone[:8000]'][k])
    assert not oracle['lead']['lag'][:30].any() and not oracle['zero']['vprob'].any()


def test_batched_rows_are_bitwise_their_own_calls_for_every_chunking(rows, oracle):
    from segan_pytorch_amd import ops
    names = [n for n, (_, srate) in rows.items() if srate == 16000]
    T = max(len(rows[n][0]) for n in names)
    X = np.full((len(names), T), np.nan, np.float32)       # NaN past every row's length
    for i, n in enumerate(names):
        X[i, :len(rows[n][0])] = rows[n][0]
    lens = [len(rows[n][0]) for n in names]
    got = ops.pyin_stages(_cuda(X), lengths=lens)
    F = P.n_frames(T, 16000)
    assert got['f0'].shape == (len(names), F) and got['bv'].shape == (len(names), F, 165)
    for i, n in enumerate(names):
        _check_row(got, i, oracle[n], n + ' (batched)')
    per_row = 8 * ops.pyin_dims(1, T)['ws_doubles']
    again = ops.pyin_stages(_cuda(X), lengths=torch.tensor(lens), ws_cap=3 * per_row + 100)
    for k in got:
        assert torch.equal(_bits(got[k].double()), _bits(again[k].double())), k
    with pytest.raises(ValueError, match='ws_cap'):
        ops.pyin(_cuda(X), lengths=lens, ws_cap=per_row - 8)
    # 8 kHz, two rows of different length in one call
    x8 = rows['tone8'][0]
    X8 = np.full((2, len(x8)), np.nan, np.float32)
    X8[0], X8[1, :1500] = x8, x8[:1500]
    got8 = ops.pyin_stages(_cuda(X8), lengths=[len(x8), 1500], srate=8000)
    _check_row(got8, 0, oracle['tone8'], 'tone8 (batched)')
    _check_row(got8, 1, Y.track(x8[:1500], 8000, tabs=ops.pyin_tables(8000)), 'tone8[:1500]')


def test_quality_takes_the_tracker_and_keeps_its_default(rows, oracle):
    from segan_pytorch_amd import ops, quality
    pfx = load_golden('pitch.pt')
    tol = {k: 100 * pfx['meta']['gaps'][k] for k in ('f0_mae', 'f0_kld')}
    pairs = [('tone[:8000]', 'lead'), ('lead', 'octave'), ('octave', 'tone*2^-10'),
             ('tone[:8000]', 'zero')]
    n = 8000
    ref = np.stack([np.resize(rows[a][0], n) if a != 'zero' else np.zeros(n, np.float32)
                    for a, _ in pairs])
    deg = np.stack([np.resize(rows[b][0], n) if b != 'zero' else np.zeros(n, np.float32)
                    for _, b in pairs])
    got = quality.f0_eval(_cuda(ref), _cuda(deg), tracker='pyin')
    assert set(got) == {'f0_mae', 'vuv_acc', 'f0_kld', 'voiced'}
    tabs = ops.pyin_tables(16000)
    zero = Y.track(np.zeros(n, np.float32), 16000, tabs=tabs)

    def contour(name):
        return zero if name == 'zero' else oracle[name]

    fr, lr, fd, ld = (_cuda(np.stack([contour(p[j])[k] for p in pairs]))
                      for j, k in ((0, 'f0'), (0, 'lag'), (1, 'f0'), (1, 'lag')))
    want = ops.f0_eval(fr, lr, fd, ld).cpu().numpy()
    for c, k in enumerate(('f0_mae', 'vuv_acc', 'f0_kld', 'voiced')):
        g = got[k].cpu().numpy()
        assert got[k].shape == (4,) and got[k].dtype == torch.float64
        for i in range(len(pairs)):
            w = want[i, c]
            print('{} vs {}: {} {!r} (on the oracle\'s contours {!r})'.format(*pairs[i], k, g[i], w))
            assert math.isnan(g[i]) == math.isnan(w), (pairs[i], k)
            if math.isnan(w):
                continue
            if k in tol:
                assert abs(g[i] - w) <= tol[k] * max(abs(w), 1.0), (pairs[i], k, g[i], w)
            else:
                assert g[i] == w, (pairs[i], k, g[i], w)
    assert math.isnan(want[3, 0]) and want[3, 1] == 0.0 and np.isfinite(want[:3]).all()
    # the third value is vprob with 'pyin'; without `tracker` nothing has changed
    x = _cuda(ref)
    f0, voiced, vp = quality.pitch(x, tracker='pyin')
    of0, olag, ovp, _ = ops.pyin(x)
    assert torch.equal(_bits(f0), _bits(of0)) and torch.equal(voiced, olag > 0)
    assert torch.equal(_bits(vp), _bits(ovp)) and voiced.dtype == torch.bool
    assert float(vp.min()) >= 0.0 and float(vp.max()) <= 1.0 + 1e-12
    yf0, ylag, yap, _ = ops.pitch(x)
    for res in (quality.pitch(x), quality.pitch(x, tracker='yin')):
        assert torch.equal(_bits(res[0]), _bits(yf0)) and torch.equal(res[1], ylag > 0)
        assert torch.equal(_bits(res[2]), _bits(yap))
    a, b = quality.f0_eval(x, _cuda(deg)), quality.f0_eval(x, _cuda(deg), tracker='yin')
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert quality.pitch(x[0], tracker='pyin')[0].shape == (1, 92)


def test_validation_errors_and_rows_without_a_frame():
    from segan_pytorch_amd import ops, quality
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.pyin, ops.pyin_stages):
        with pytest.raises(TypeError):
            fn(x.double())
        with pytest.raises(ValueError, match='srate'):
            fn(x, srate=44100)
        with pytest.raises(ValueError, match='lengths'):
            fn(x, lengths=[5000, 5001])
        with pytest.raises(ValueError, match='ws_cap'):
            fn(x, ws_cap=0)
    with pytest.raises(ValueError, match='tracker'):
        quality.pitch(x, tracker='swipe')
    got = ops.pyin_stages(x[:, :600].contiguous())
    assert got['f0'].shape == got['state'].shape == (2, 0) and got['bv'].shape == (2, 0, 165)
    assert got['nframes'].tolist() == [0, 0] and torch.isnan(got['delta']).all()
    short = quality.f0_eval(x[:, :600], x[:, :600], tracker='pyin')
    assert all(torch.isnan(v).all() and v.shape == (2,) for v in short.values())
    f0, lag, vp, nfr = ops.pyin(x, lengths=[5000, 0])
    assert nfr.tolist() == [P.n_frames(5000, 16000), 0]
    assert (lag[1] == -1).all() and not f0[1].any() and torch.isnan(vp[1]).all()


def _fake_pesqmain(tmp_path):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\necho "P.862 Prediction (Raw MOS, MOS-LQO):  = 1.0\t2.500"\n')
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_eval_cli_prints_the_same_columns_with_either_tracker(rows, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import quality
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    clean, noisy = rows['tone[:8000]'][0][:6000], rows['lead'][0][:6000]
    wavfile.write(str(cdir / 'a.wav'), 16000, clean)
    wavfile.write(str(ndir / 'a.wav'), 16000, noisy)
    env = dict(os.environ)
    env['PATH'] = _fake_pesqmain(tmp_path) + os.pathsep + env['PATH']
    lines = {}
    for tracker in ('yin', 'pyin'):
        log = tmp_path / (tracker + '.log')
        p = subprocess.run(['timeout', '-k', '10', '120', sys.executable,
                            os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs',
                            str(ndir), '--clean_wavs', str(cdir), '--logfile', str(log), '--f0'] +
                           (['--f0_tracker', 'pyin'] if tracker == 'pyin' else []),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, cwd=ROOT,
                           universal_newlines=True)
        assert p.returncode == 0, p.stdout
        assert 'mean F0MAE: ' in p.stdout and 'mean VUV: ' in p.stdout
        lines[tracker] = log.read_text().splitlines()
        r = quality.f0_eval(_cuda(clean), _cuda(noisy), tracker=tracker)
        want = ['{:.4f}'.format(float(r[k])) for k in ('f0_mae', 'vuv_acc', 'f0_kld')]
        assert lines[tracker][1].split()[6:] == want, (tracker, lines[tracker])
    assert lines['yin'][0] == lines['pyin'][0] == 'FILE CSIG CBAK COVL PESQ SSNR F0MAE VUV F0KLD'
    assert len(lines['yin']) == len(lines['pyin']) == 2
    assert lines['yin'][1].split()[:6] == lines['pyin'][1].split()[:6]
