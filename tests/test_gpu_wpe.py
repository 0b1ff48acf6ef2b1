"""The WPE dereverberation baseline on the MI355X (ops.wpe_rows / wpe_stages, baselines.wpe,
clean.py --wpe, eval_noisy_performance.py --wpe) against the numpy oracle scripts/wpe_oracle.py and
its fixture tests/golden/wpe.pt.

Decisions: `nframes` and `status` are compared exactly.

Tolerances: for each case, 100 x the movement of the oracle between float64 and numpy.longdouble
on that very row, as scripts/make_golden_wpe.py recorded it in the fixture (case.gaps): y relative
to max |x| of the row, X relative to max |Y|, g absolute.  The kernels' rounding is of the oracle's
class; the factor covers another FFT and the ascending order of the sums over the frames.  The
reference of every case is the float64 oracle, run once per module (its subsample is checked
against the fixture's by tests/test_wpe.py).  The three rows around the kernel's frame tile of 512
frames are taken at 8 kHz, where 513 frames are 4.1 s.

The figures measured on an MI355X are in README.md and DESIGN.md section 21; each test prints its
own."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import wpe_oracle as O  # noqa: E402
import make_golden_wpe as GW  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def wfx():
    return load_golden('wpe.pt')


@pytest.fixture(scope='module')
def rows(wfx):
    return GW.case_rows({k: v.numpy() for k, v in wfx['signals'].items()})


@pytest.fixture(scope='module')
def oracle(rows):
    """case -> the float64 oracle's run, computed once."""
    return {name: O.wpe(x, srate, **kw) for name, (x, srate, kw) in rows.items()}


def _bits(t):
    t = t.contiguous()
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _row_of(got, i, L, nf):
    """Row i of a dict of ops.wpe_stages as the oracle's dict, frames past the row's own checked
    to be zero."""
    y = got['y'][i] if got['y'].dim() == 2 else got['y']
    Y, X = got['Y'][i].cpu().numpy(), got['X'][i].cpu().numpy()
    assert not Y[:, nf:].any() and not X[:, nf:].any() and not y[L:].any()
    return {'y': y[:L].cpu().numpy(), 'Y': Y[:, :nf], 'X': X[:, :nf], 'g': got['g'][i].cpu().numpy()}


def _check(wfx, oracle, name, x, got, i=0):
    want, ref = wfx['cases'][name], oracle[name]
    nf = want['nframes']
    assert int(got['nframes'][i]) == nf == ref['nframes']
    assert int(got['status'][i]) == want['status'] == ref['status']
    r = _row_of(got, i, len(x), nf)
    for k in ('y', 'X', 'g'):
        assert np.isfinite(r[k].view(np.float64)).all(), (name, k)
    err = GW.errors(r, ref, x)
    err['Y'] = float(np.abs(r['Y'] - ref['Y']).max() / max(np.abs(ref['Y']).max(), 1e-300))
    print('{:14s} frames {:3d}: '.format(name, nf) + ', '.join(
        '{} {:.3g} (tolerance {:.3g})'.format(k, err[k], 100 * want['gaps'][k])
        for k in ('y', 'X', 'g')) + ', Y {:.3g}'.format(err['Y']))
    for k in ('y', 'X', 'g'):
        assert err[k] <= 100 * want['gaps'][k], (name, k, err[k], want['gaps'][k])
    return err


def test_every_case_matches_the_oracle(wfx, rows, oracle):
    from segan_pytorch_amd import ops
    for name, (x, srate, kw) in rows.items():
        got = ops.wpe_stages(_cuda(x), srate=srate, out_dtype=torch.float64, **kw)
        N, H, F = O.constants(srate)
        nf = O.n_frames(len(x), srate)
        assert got['y'].shape == (len(x),) and got['y'].dtype == torch.float64
        assert got['Y'].shape == got['X'].shape == (1, F, nf) and got['g'].shape == (1, F, kw['taps'])
        assert got['Y'].dtype == got['X'].dtype == got['g'].dtype == torch.complex128
        assert got['nframes'].dtype == got['status'].dtype == torch.int32
        assert ops.wpe_dims(1, len(x), srate)['frames'] == nf
        _check(wfx, oracle, name, x, got)
    # the rows of at most delay + taps frames are the input, bit for bit, in either dtype
    for name in ('L1', 'L127', 'L128', 'L129', 'L1280'):
        x = _cuda(rows[name][0])
        assert torch.equal(_bits(ops.wpe_rows(x)), _bits(x)), name
        assert torch.equal(_bits(ops.wpe_rows(x.double())), _bits(x.double())), name
    x = _cuda(rows['L1281'][0])
    assert not torch.equal(_bits(ops.wpe_rows(x)), _bits(x))
    assert torch.equal(_bits(ops.wpe_rows(x, delay=4)), _bits(x))
    # zero in, zero out
    z = ops.wpe_stages(_cuda(rows['zero'][0]))
    assert not z['y'].any() and not torch.view_as_real(z['g']).any() and int(z['status'][0]) == 0


def test_a_power_of_two_scales_every_bit(rows):
    from segan_pytorch_amd import ops
    a = ops.wpe_stages(_cuda(rows['L8000'][0]), out_dtype=torch.float64)
    b = ops.wpe_stages(_cuda(rows['scaled'][0]), out_dtype=torch.float64)
    assert torch.equal(_bits(b['y'] * 1024.0), _bits(a['y']))
    assert torch.equal(_bits(b['X'] * 1024.0), _bits(a['X']))
    assert torch.equal(_bits(b['g']), _bits(a['g']))


def _ragged(rows):
    """the 16 kHz cases with the default parameters in one batch, NaN past each length"""
    names = [n for n, (x, srate, kw) in rows.items() if srate == 16000 and kw == GW.DEFAULTS]
    T = max(len(rows[n][0]) for n in names) + 777
    X = np.full((len(names), T), np.nan, np.float32)
    for i, n in enumerate(names):
        X[i, :len(rows[n][0])] = rows[n][0]
    return names, _cuda(X), [len(rows[n][0]) for n in names]


def test_a_batched_row_is_bitwise_its_own_call_for_every_chunking(wfx, rows, oracle):
    from segan_pytorch_amd import baselines, ops
    names, X, lens = _ragged(rows)
    assert 'L1' in names and 'L32000' in names and 'band4k' in names and len(names) == 12
    got = ops.wpe_stages(X, lengths=lens, out_dtype=torch.float64)
    nfT = O.n_frames(X.shape[1])
    assert got['y'].shape == X.shape and got['X'].shape == (len(names), 257, nfT)
    for i, n in enumerate(names):
        _check(wfx, oracle, n, rows[n][0], got, i)
        one = ops.wpe_stages(_cuda(rows[n][0]), out_dtype=torch.float64)
        nf = one['X'].shape[2]
        assert torch.equal(_bits(one['y']), _bits(got['y'][i, :lens[i]])), n
        for k in ('Y', 'X'):
            assert torch.equal(_bits(one[k][0]), _bits(got[k][i, :, :nf])), (n, k)
        assert torch.equal(_bits(one['g'][0]), _bits(got['g'][i])), n
        assert int(one['nframes'][0]) == int(got['nframes'][i])
    per_row = ops.wpe_dims(1, X.shape[1])['ws_bytes']
    assert per_row == 32 * 257 * nfT + 4 * 260
    again = ops.wpe_stages(X, lengths=torch.tensor(lens), out_dtype=torch.float64,
                           ws_cap=3 * per_row + 100)
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(again[k])), k
    with pytest.raises(ValueError, match='ws_cap'):
        ops.wpe_rows(X, lengths=lens, ws_cap=per_row - 8)
    y = ops.wpe_rows(X, lengths=lens, out_dtype=torch.float64)
    assert torch.equal(_bits(y), _bits(got['y']))
    Xd = torch.nan_to_num(X).double()
    assert torch.equal(_bits(baselines.wpe(Xd, 16000, lens)), _bits(y))


def test_the_tile_does_not_show_in_a_longer_buffer(rows):
    """A row of 513 frames alone (two tiles) and as the head of a longer buffer: the same bits."""
    from segan_pytorch_amd import ops
    x = rows['tile8_L32577'][0]
    one = ops.wpe_stages(_cuda(x), srate=8000, out_dtype=torch.float64)
    pad = np.full(len(x) + 5000, np.nan, np.float32)
    pad[:len(x)] = x
    two = ops.wpe_stages(_cuda(pad), lengths=[len(x)], srate=8000, out_dtype=torch.float64)
    assert torch.equal(_bits(one['y']), _bits(two['y'][:len(x)]))
    assert torch.equal(_bits(one['g']), _bits(two['g']))
    assert torch.equal(_bits(one['X'][0]), _bits(two['X'][0, :, :513]))


def test_output_dtypes_round_once(rows):
    from segan_pytorch_amd import ops
    names, X, lens = _ragged(rows)
    y64 = ops.wpe_rows(X, lengths=lens, out_dtype=torch.float64)
    y32 = ops.wpe_rows(X, lengths=lens)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    assert torch.equal(_bits(y32), _bits(y64.float()))
    # an fp64 input of the same values gives the same bits; its default output is fp64
    Xd = torch.nan_to_num(X).double()
    d64 = ops.wpe_rows(Xd, lengths=lens)
    assert d64.dtype == torch.float64 and torch.equal(_bits(d64), _bits(y64))
    assert torch.equal(_bits(ops.wpe_rows(Xd, lengths=lens, out_dtype=torch.float32)), _bits(y32))
    x8 = _cuda(rows['rate8'][0])
    a = ops.wpe_rows(x8, srate=8000, out_dtype=torch.float64)
    assert torch.equal(_bits(ops.wpe_rows(x8, srate=8000)), _bits(a.float()))


def test_validation_errors():
    from segan_pytorch_amd import baselines, ops
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.wpe_rows, ops.wpe_stages):
        with pytest.raises(TypeError):
            fn(x.half())
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu())
        with pytest.raises(ValueError, match='srate'):
            fn(x, srate=44100)
        with pytest.raises(ValueError, match='taps'):
            fn(x, taps=33)
        with pytest.raises(ValueError, match='lengths'):
            fn(x, lengths=[5000, 5001])
    with pytest.raises(RuntimeError, match='MI355X'):
        baselines.wpe(x.cpu())
    short = x[:, :1000].contiguous()
    st = ops.wpe_stages(short)                    # 11 frames: every row is copied
    assert st['nframes'].tolist() == [11, 11] and st['status'].tolist() == [0, 0]
    assert torch.equal(st['y'], short) and not torch.view_as_real(st['g']).any()


def test_srmr_before_and_after_is_reported(wfx):
    """SRMR of the fixture's reverberant signals before and after WPE: printed, not asserted."""
    from segan_pytorch_amd import baselines, quality
    for name in ('rev03', 'rev06'):
        x = _cuda(GW.row(wfx['signals'][name].numpy()))
        y = baselines.wpe(x)
        assert y.shape == x.shape and y.dtype == torch.float32 and torch.isfinite(y).all()
        print('{}: SRMR {:.4f} before, {:.4f} after WPE'.format(
            name, float(quality.srmr(x)[0]), float(quality.srmr(y)[0])))


def _run(args):
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    return p.stdout


def test_clean_cli_wpe_writes_the_inputs_dtype_rate_and_length(wfx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import baselines
    from segan_pytorch_amd.resample import resample_wav
    src, dst, dst2 = tmp_path / 'in', tmp_path / 'out', tmp_path / 'out2'
    for d in (src, dst, dst2):
        d.mkdir()
    f16 = GW.row(wfx['signals']['rev06'].numpy())[:12000].copy()
    i8 = wfx['signals']['rev8'].numpy()[:8000].copy()
    wavfile.write(str(src / 'a.wav'), 16000, f16)
    wavfile.write(str(src / 'b.wav'), 8000, i8)
    out = _run([os.path.join(ROOT, 'clean.py'), '--wpe', '--test_files', str(src),
                '--synthesis_path', str(dst), '--cuda', '--resample', '--keep_rate', '--srmr'])
    assert 'Cleaning 2 wavs' in out and 'mean SRMR' in out
    rate, a = wavfile.read(str(dst / 'a.wav'))
    assert rate == 16000 and a.dtype == np.float32 and a.shape == f16.shape
    assert np.array_equal(a, baselines.wpe(_cuda(f16)).cpu().numpy())
    assert np.array_equal(a, baselines.wpe_wav(f16))
    rate, b = wavfile.read(str(dst / 'b.wav'))
    assert rate == 8000 and b.dtype == np.int16 and b.shape == i8.shape
    up = resample_wav(i8, 8000, 16000)
    assert up.dtype == np.int16
    y = baselines.wpe(_cuda(up.astype(np.float32) / 32768).double()).cpu().numpy()
    y16 = np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(y16, baselines.wpe_wav(up))
    assert np.array_equal(b, resample_wav(y16, 16000, 8000)[:len(i8)])
    assert np.abs(b.astype(np.float64)).max() > 100 and not np.array_equal(b, i8)
    # the parameters reach the kernel, and WPE runs before the denoiser
    _run([os.path.join(ROOT, 'clean.py'), '--wpe', '--wpe_taps', '4', '--wpe_delay', '2',
          '--wpe_iterations', '1', '--baseline', 'wiener', '--test_files', str(src / 'a.wav'),
          '--synthesis_path', str(dst2), '--cuda'])
    rate, c = wavfile.read(str(dst2 / 'a.wav'))
    w = baselines.wpe_wav(f16, taps=4, delay=2, iterations=1)
    assert not np.array_equal(w, a)
    assert np.array_equal(c, baselines.denoise_wav(w, 'wiener'))


def test_eval_cli_wpe_measures_the_dereverberated_signal(wfx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import baselines
    from segan_pytorch_amd.quality import composite_eval
    cdir, ndir = tmp_path / 'clean', tmp_path / 'rev'
    cdir.mkdir()
    ndir.mkdir()
    early, rev = (GW.row(wfx['signals'][k].numpy()) for k in ('early06', 'rev06'))
    want, both = {}, {}
    for name, L in (('a.wav', 32000), ('b.wav', 20000)):
        wavfile.write(str(cdir / name), 16000, early[:L])
        wavfile.write(str(ndir / name), 16000, rev[:L])
        y = baselines.wpe(_cuda(rev[:L]))
        assert y.dtype == torch.float32
        want[name] = float(composite_eval(_cuda(early[:L]), y)['ssnr'][0])
        both[name] = float(composite_eval(_cuda(early[:L]), baselines.wiener(y))['ssnr'][0])
        plain = float(composite_eval(_cuda(early[:L]), _cuda(rev[:L]))['ssnr'][0])
        print('{}: SSNR against the early target {:.3f} dB, after WPE {:.3f} dB'.format(
            name, plain, want[name]))
        assert '{:.3}'.format(want[name]) != '{:.3}'.format(plain)
    for flags, expect in ((['--wpe'], want), (['--wpe', '--baseline', 'wiener'], both)):
        log = tmp_path / 'eval.log'
        _run([os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
              '--clean_wavs', str(cdir), '--logfile', str(log)] + flags)
        lines = log.read_text().splitlines()
        assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR'
        assert [l.split()[0] for l in lines[1:]] == ['a.wav', 'b.wav']
        for line in lines[1:]:
            f = line.split()
            assert len(f) == 6 and f[5] == '{:.3}'.format(expect[f[0]]), line
