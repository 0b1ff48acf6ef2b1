"""The Wiener / log-MMSE baseline enhancers on the MI355X (ops.denoise_rows / denoise_stages,
baselines, clean.py --baseline, eval_noisy_performance.py --baseline) against the numpy oracle
scripts/denoise_oracle.py and its fixture tests/golden/denoise.pt.

Decisions.  No frame of the fixture has |v_t - 0.15| below 1e-7 (the smallest is 1.8e-3), eight
orders of magnitude above the rounding of v_t, so `nframes` and the noise-update flag of every
frame are compared exactly with the fixture's, with no exemption.

Tolerances: 100 x the movement of the oracle between float64 and numpy.longdouble, per rule and
quantity, as scripts/make_golden_denoise.py measured it (meta.gaps): y relative to max |x| of the
row, 1.2e-13 for either rule; v_t relative to max(1, |v_t|), 1.1e-13 (wiener) and 1.3e-13
(logmmse).  v_t is compared with the fixture's; y with the fixture's where it is stored (rows up to
2080 samples) and with the oracle run once per module otherwise.

Measured on an MI355X (each test prints its figures): every decision equal; y at most 1.33e-15
(wiener, the row that starts in silence) and 1.14e-15 (logmmse) of max |x|; v_t at most 8.9e-16 and
9.6e-16; batching, chunking and the output dtypes bit-equal.  The tolerances stay as asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import denoise_oracle as O  # noqa: E402
import make_golden_denoise as GD  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ['L1919', 'L1920', 'L2079', 'L2080', 'L8000', 'L32000', 'rate8', 'zero', 'silent_start',
         'scaled']


@pytest.fixture(scope='module')
def dfx():
    return load_golden('denoise.pt')


@pytest.fixture(scope='module')
def rows(dfx):
    return GD.case_rows(dfx['signals'])


@pytest.fixture(scope='module')
def oracle_y(dfx, rows):
    """(case, rule) -> the oracle's y, computed once: stored for the short rows, run here for the
    others (its decisions are asserted to be the fixture's)."""
    out = {}
    for name, (x, srate) in rows.items():
        for rule in O.RULES:
            want = dfx['cases'][name][rule]
            if 'y' in want:
                out[name, rule] = want['y'].numpy()
            else:
                r = O.denoise(x, srate, rule)
                assert np.array_equal(r['update'], want['update'].numpy())
                out[name, rule] = r['y']
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _distances(dfx, got, i, name, rule, x, want_y):
    """row i of a dict of ops.denoise_stages against the fixture: decisions exactly, the distances
    of y and v_t returned"""
    want = dfx['cases'][name][rule]
    nf = want['nframes']
    assert int(got['nframes'][i]) == nf
    upd = got['noise_update'][i].cpu().numpy()
    vad = got['vad'][i].cpu().numpy()
    assert np.array_equal(upd[:nf], want['update'].numpy().astype(np.int32)), (name, rule)
    assert (upd[nf:] == -1).all() and np.isnan(vad[nf:]).all()
    y = got['y'][i].cpu().numpy() if got['y'].dim() == 2 else got['y'].cpu().numpy()
    L = len(x)
    assert np.isfinite(y).all() and not y[L:].any()
    peak = float(np.abs(x).max())
    if peak == 0:
        assert not y.any()
        dy = 0.0
    else:
        dy = float(np.abs(y[:L] - want_y).max()) / peak
    dv = 0.0
    if nf:
        w = want['vad'].numpy()
        dv = float(np.max(np.abs(vad[:nf] - w) / np.maximum(1.0, np.abs(w))))
    return dy, dv


@pytest.mark.parametrize('rule', O.RULES)
def test_every_case_matches_the_oracle(dfx, rows, oracle_y, rule):
    from segan_pytorch_amd import ops
    tol = {k: 100 * v for k, v in dfx['meta']['gaps'][rule].items()}
    worst = {'y': 0.0, 'vad': 0.0}
    for name in CASES:
        x, srate = rows[name]
        got = ops.denoise_stages(_cuda(x), srate=srate, rule=rule, out_dtype=torch.float64)
        assert got['y'].shape == (len(x),) and got['y'].dtype == torch.float64
        nfmax = O.n_frames(len(x), srate)
        assert got['vad'].shape == got['noise_update'].shape == (1, nfmax)
        assert got['nframes'].dtype == got['noise_update'].dtype == torch.int32
        dy, dv = _distances(dfx, got, 0, name, rule, x, oracle_y[name, rule])
        print('{:7s} {:12s} frames {:3d}: y {:.3g} (tolerance {:.3g}), v_t {:.3g} (tolerance '
              '{:.3g})'.format(rule, name, int(got['nframes'][0]), dy, tol['y'], dv, tol['vad']))
        worst = {'y': max(worst['y'], dy), 'vad': max(worst['vad'], dv)}
    print('{}: worst y {:.3g}, v_t {:.3g}'.format(rule, worst['y'], worst['vad']))
    assert worst['y'] <= tol['y'] and worst['vad'] <= tol['vad'], worst
    # the short row is the input, bit for bit, in either dtype
    x = _cuda(rows['L1919'][0])
    assert torch.equal(_bits(ops.denoise_rows(x, rule=rule)), _bits(x))
    assert torch.equal(_bits(ops.denoise_rows(x.double(), rule=rule)), _bits(x.double()))


def _ragged(rows):
    """the 16 kHz cases in one batch, garbage past each length"""
    names = [n for n in CASES if rows[n][1] == 16000]
    T = max(len(rows[n][0]) for n in names)
    X = np.random.default_rng(5).standard_normal((len(names), T)).astype(np.float32)
    for i, n in enumerate(names):
        X[i, :len(rows[n][0])] = rows[n][0]
    return names, _cuda(X), [len(rows[n][0]) for n in names]


@pytest.mark.parametrize('rule', O.RULES)
def test_a_batched_row_is_bitwise_its_own_call_for_every_chunking(dfx, rows, oracle_y, rule):
    from segan_pytorch_amd import baselines, ops
    names, X, lens = _ragged(rows)
    got = ops.denoise_stages(X, lengths=lens, rule=rule, out_dtype=torch.float64)
    assert got['y'].shape == X.shape and got['vad'].shape == (len(names), 199)
    tol = {k: 100 * v for k, v in dfx['meta']['gaps'][rule].items()}
    for i, n in enumerate(names):
        dy, dv = _distances(dfx, got, i, n, rule, rows[n][0], oracle_y[n, rule])
        assert dy <= tol['y'] and dv <= tol['vad'], (n, dy, dv)
        nf = dfx['cases'][n][rule]['nframes']
        if nf:      # zero from (nf + 1) H on, whatever lies past the length
            assert not got['y'][i, (nf + 1) * 160:].any()
        one = ops.denoise_stages(_cuda(rows[n][0]), rule=rule, out_dtype=torch.float64)
        assert torch.equal(_bits(one['y']), _bits(got['y'][i, :lens[i]])), n
        assert torch.equal(_bits(one['vad'][0]), _bits(got['vad'][i, :one['vad'].shape[1]])), n
        assert torch.equal(one['noise_update'][0].cpu(),
                           got['noise_update'][i, :one['vad'].shape[1]].cpu())
    per_row = ops.denoise_dims(1, X.shape[1])['ws_bytes']
    assert per_row == 16 * 321 * 199 + 8 * 321
    again = ops.denoise_stages(X, lengths=torch.tensor(lens), rule=rule, out_dtype=torch.float64,
                               ws_cap=3 * per_row + 100)
    for k in got:
        assert torch.equal(_bits(got[k].double()), _bits(again[k].double())), k
    with pytest.raises(ValueError, match='ws_cap'):
        ops.denoise_rows(X, lengths=lens, ws_cap=per_row - 8)
    y = ops.denoise_rows(X, lengths=lens, rule=rule, out_dtype=torch.float64)
    assert torch.equal(_bits(y), _bits(got['y']))
    assert torch.equal(_bits(baselines.denoise(X.double(), 16000, lens, rule)), _bits(y))
    fn = baselines.wiener if rule == 'wiener' else baselines.logmmse
    assert torch.equal(_bits(fn(X.double(), lengths=lens)), _bits(y))


def test_output_dtypes_round_once(rows):
    from segan_pytorch_amd import ops
    names, X, lens = _ragged(rows)
    for rule in O.RULES:
        y64 = ops.denoise_rows(X, lengths=lens, rule=rule, out_dtype=torch.float64)
        y32 = ops.denoise_rows(X, lengths=lens, rule=rule)
        assert y32.dtype == torch.float32 and y64.dtype == torch.float64
        assert torch.equal(_bits(y32), _bits(y64.float()))
        # an fp64 input of the same values gives the same bits; its default output is fp64
        d64 = ops.denoise_rows(X.double(), lengths=lens, rule=rule)
        assert d64.dtype == torch.float64 and torch.equal(_bits(d64), _bits(y64))
        d32 = ops.denoise_rows(X.double(), lengths=lens, rule=rule, out_dtype=torch.float32)
        assert torch.equal(_bits(d32), _bits(y32))
    x8 = _cuda(rows['rate8'][0])
    a = ops.denoise_rows(x8, srate=8000, out_dtype=torch.float64)
    assert torch.equal(_bits(ops.denoise_rows(x8, srate=8000)), _bits(a.float()))


def test_validation_errors():
    from segan_pytorch_amd import baselines, ops
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.denoise_rows, ops.denoise_stages):
        with pytest.raises(TypeError):
            fn(x.half())
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu())
        with pytest.raises(ValueError, match='srate'):
            fn(x, srate=44100)
        with pytest.raises(ValueError, match='rule'):
            fn(x, rule='mmse')
        with pytest.raises(ValueError, match='lengths'):
            fn(x, lengths=[5000, 5001])
    with pytest.raises(RuntimeError, match='MI355X'):
        baselines.logmmse(x.cpu())
    short = x[:, :1000].contiguous()
    st = ops.denoise_stages(short)                # no row has a frame: everything is copied
    assert st['nframes'].tolist() == [0, 0] and st['vad'].shape == (2, 0)
    assert torch.equal(st['y'], short)


def _run(args):
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    return p.stdout


def test_clean_cli_baseline_writes_the_inputs_dtype_rate_and_length(dfx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import baselines
    from segan_pytorch_amd.resample import resample_wav
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    dst.mkdir()
    f16 = dfx['signals']['noisy'].numpy()[:12000]
    i8 = np.clip(np.rint(dfx['signals']['noisy8'].numpy().astype(np.float64) * 32768 * 4),
                 -32768, 32767).astype(np.int16)
    wavfile.write(str(src / 'a.wav'), 16000, f16)
    wavfile.write(str(src / 'b.wav'), 8000, i8)
    out = _run([os.path.join(ROOT, 'clean.py'), '--baseline', 'logmmse', '--test_files', str(src),
                '--synthesis_path', str(dst), '--cuda', '--resample', '--keep_rate'])
    assert 'Cleaning 2 wavs' in out
    rate, a = wavfile.read(str(dst / 'a.wav'))
    assert rate == 16000 and a.dtype == np.float32 and a.shape == f16.shape
    assert np.array_equal(a, baselines.logmmse(_cuda(f16)).cpu().numpy())
    rate, b = wavfile.read(str(dst / 'b.wav'))
    assert rate == 8000 and b.dtype == np.int16 and b.shape == i8.shape
    up = resample_wav(i8, 8000, 16000)
    assert up.dtype == np.int16
    y = baselines.logmmse(_cuda(up.astype(np.float32) / 32768).double()).cpu().numpy()
    y16 = np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)
    assert np.array_equal(b, resample_wav(y16, 16000, 8000)[:len(i8)])
    assert np.abs(b.astype(np.float64)).max() > 100 and not np.array_equal(b, i8)


def test_eval_cli_baseline_measures_the_enhanced_signal(dfx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import baselines
    from segan_pytorch_amd.quality import composite_eval
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    clean, noisy = (dfx['signals'][k].numpy() for k in ('clean', 'noisy'))
    want = {}
    for name, L in (('a.wav', 32000), ('b.wav', 20000)):
        wavfile.write(str(cdir / name), 16000, clean[:L])
        wavfile.write(str(ndir / name), 16000, noisy[:L])
        enh = baselines.wiener(_cuda(noisy[:L]))
        assert enh.dtype == torch.float32
        r = composite_eval(_cuda(clean[:L]), enh)
        plain = composite_eval(_cuda(clean[:L]), _cuda(noisy[:L]))
        want[name] = float(r['ssnr'][0])
        assert want[name] > float(plain['ssnr'][0])
    log = tmp_path / 'eval.log'
    _run([os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
          '--clean_wavs', str(cdir), '--logfile', str(log), '--baseline', 'wiener'])
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR'
    assert [l.split()[0] for l in lines[1:]] == ['a.wav', 'b.wav']
    for line in lines[1:]:
        f = line.split()
        assert len(f) == 6 and f[5] == '{:.3}'.format(want[f[0]]), line
