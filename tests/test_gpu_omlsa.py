"""The OM-LSA enhancer with IMCRA noise tracking on the MI355X (ops.omlsa_rows / omlsa_stages,
baselines.omlsa, clean.py --omlsa, eval_noisy_performance.py --omlsa) against the numpy oracle
scripts/omlsa_oracle.py and its fixture tests/golden/omlsa.pt.

Decisions.  No discontinuous comparison of any bin and frame of the fixture (s2 against g0 th, S
against z0 th, St against z0 tth) is closer than 3.0e-6 relative, nine orders of magnitude above
the rounding of its two sides, so `nframes` and the rough count of every frame are compared
exactly with the fixture's, with no exemption.

Tolerances: 100 x the movement of the oracle between float64 and numpy.longdouble per quantity, as
scripts/make_golden_omlsa.py measured it (meta.gaps): y relative to max |x| of the row, 1.6e-13;
presence absolute, 4.5e-14; the noise spectrum relative to its own maximum, 2.5e-13.  presence,
rough and noise are compared with the fixture's; y with the fixture's where it is stored (rows up
to 2080 samples) and with the oracle run once per module otherwise.

Measured on an MI355X (each test prints its figures): every frame count and rough count equal; y
at most 1.41e-15 of max |x| (step_up), presence 4.44e-16 (step_up), noise 1.53e-15 of its maximum
(L = 1920); batching, chunking and the output dtypes bit-equal; the late-voiced SNR of omlsa on
step_up / ramp / step_down 7.69 / 8.89 / 11.31 dB against 6.80 / 6.92 / 6.75 (wiener) and 6.49 /
6.64 / 7.52 (logmmse).  The tolerances stay as asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_omlsa as GO  # noqa: E402
import omlsa_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ['L1919', 'L1920', 'L2079', 'L2080', 'L8000', 'L32000', 'rate8', 'zero', 'silent_start',
         'scaled', 'flat', 'step_up', 'step_down', 'ramp']
CHANGING = ('step_up', 'ramp', 'step_down')


@pytest.fixture(scope='module')
def ofx():
    return load_golden('omlsa.pt')


@pytest.fixture(scope='module')
def rows(ofx):
    return GO.case_rows({k: v.numpy() for k, v in ofx['signals'].items()}, ofx['gains'])


@pytest.fixture(scope='module')
def oracle_y(ofx, rows):
    """case -> the oracle's y, computed once: stored for the short rows, run here for the others
    (its rough counts are asserted to be the fixture's)."""
    out = {}
    for name, (x, srate) in rows.items():
        want = ofx['cases'][name]
        if 'y' in want:
            out[name] = want['y'].numpy()
        else:
            r = O.omlsa(x, srate)
            assert np.array_equal(r['rough'], want['rough'].numpy())
            out[name] = r['y']
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32).cpu()


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _distances(ofx, got, i, name, x, want_y):
    """row i of a dict of ops.omlsa_stages against the fixture: the frame count and every rough
    count exactly, the distances of y, presence and noise returned"""
    want = ofx['cases'][name]
    nf = want['nframes']
    assert int(got['nframes'][i]) == nf
    rough = got['rough'][i].cpu().numpy()
    pres = got['presence'][i].cpu().numpy()
    noise = got['noise'][i].cpu().numpy()
    assert np.array_equal(rough[:nf], want['rough'].numpy().astype(np.int32)), name
    assert (rough[nf:] == -1).all() and np.isnan(pres[nf:]).all()
    y = got['y'][i].cpu().numpy() if got['y'].dim() == 2 else got['y'].cpu().numpy()
    L = len(x)
    assert np.isfinite(y).all() and not y[L:].any()
    peak = float(np.abs(x).max())
    if peak == 0:
        assert not y.any()
        dy = 0.0
    else:
        dy = float(np.abs(y[:L] - want_y).max()) / peak
    if nf == 0:
        assert np.isnan(noise).all()
        return dy, 0.0, 0.0
    assert np.isfinite(pres[:nf]).all() and np.isfinite(noise).all()
    w = want['noise'].numpy()
    return (dy, float(np.abs(pres[:nf] - want['presence'].numpy()).max()),
            float(np.abs(noise - w).max() / w.max()))


def test_every_case_matches_the_oracle(ofx, rows, oracle_y):
    from segan_pytorch_amd import ops
    tol = {k: 100 * v for k, v in ofx['meta']['gaps'].items()}
    worst = {'y': 0.0, 'presence': 0.0, 'noise': 0.0}
    for name in CASES:
        x, srate = rows[name]
        got = ops.omlsa_stages(_cuda(x), srate=srate, out_dtype=torch.float64)
        assert got['y'].shape == (len(x),) and got['y'].dtype == torch.float64
        nfmax = O.n_frames(len(x), srate)
        assert got['presence'].shape == got['rough'].shape == (1, nfmax)
        assert got['noise'].shape == (1, srate // 50 + 1)
        assert got['nframes'].dtype == got['rough'].dtype == torch.int32
        assert got['presence'].dtype == got['noise'].dtype == torch.float64
        dy, dp, dn = _distances(ofx, got, 0, name, x, oracle_y[name])
        print('{:12s} frames {:3d}: y {:.3g} (tolerance {:.3g}), presence {:.3g} (tolerance '
              '{:.3g}), noise {:.3g} (tolerance {:.3g})'.format(
                  name, int(got['nframes'][0]), dy, tol['y'], dp, tol['presence'], dn,
                  tol['noise']))
        worst = {'y': max(worst['y'], dy), 'presence': max(worst['presence'], dp),
                 'noise': max(worst['noise'], dn)}
    print('worst y {y:.3g}, presence {presence:.3g}, noise {noise:.3g}'.format(**worst))
    for k in worst:
        assert worst[k] <= tol[k], (k, worst, tol)
    # the short row is the input, bit for bit, in either dtype
    x = _cuda(rows['L1919'][0])
    assert torch.equal(_bits(ops.omlsa_rows(x)), _bits(x))
    assert torch.equal(_bits(ops.omlsa_rows(x.double())), _bits(x.double()))


def _ragged(rows):
    """the 16 kHz cases in one batch, garbage past each length"""
    names = [n for n in CASES if rows[n][1] == 16000]
    T = max(len(rows[n][0]) for n in names)
    X = np.random.default_rng(5).standard_normal((len(names), T)).astype(np.float32)
    for i, n in enumerate(names):
        X[i, :len(rows[n][0])] = rows[n][0]
    return names, _cuda(X), [len(rows[n][0]) for n in names]


def test_a_batched_row_is_bitwise_its_own_call_for_every_chunking(ofx, rows, oracle_y):
    from segan_pytorch_amd import baselines, ops
    names, X, lens = _ragged(rows)
    got = ops.omlsa_stages(X, lengths=lens, out_dtype=torch.float64)
    assert got['y'].shape == X.shape and got['presence'].shape == (len(names), 399)
    assert got['noise'].shape == (len(names), 321)
    tol = {k: 100 * v for k, v in ofx['meta']['gaps'].items()}
    for i, n in enumerate(names):
        dy, dp, dn = _distances(ofx, got, i, n, rows[n][0], oracle_y[n])
        assert dy <= tol['y'] and dp <= tol['presence'] and dn <= tol['noise'], (n, dy, dp, dn)
        nf = ofx['cases'][n]['nframes']
        if nf:      # zero from (nf + 1) H on, whatever lies past the length
            assert not got['y'][i, (nf + 1) * 160:].any()
        one = ops.omlsa_stages(_cuda(rows[n][0]), out_dtype=torch.float64)
        f1 = one['presence'].shape[1]
        assert torch.equal(_bits(one['y']), _bits(got['y'][i, :lens[i]])), n
        assert torch.equal(_bits(one['presence'][0]), _bits(got['presence'][i, :f1])), n
        assert torch.equal(one['rough'][0].cpu(), got['rough'][i, :f1].cpu()), n
        assert torch.equal(_bits(one['noise'][0]), _bits(got['noise'][i])), n
    per_row = ops.omlsa_dims(1, X.shape[1])['ws_bytes']
    assert per_row == 16 * 321 * 399
    again = ops.omlsa_stages(X, lengths=torch.tensor(lens), out_dtype=torch.float64,
                             ws_cap=3 * per_row + 100)
    for k in got:
        assert torch.equal(_bits(got[k].double()), _bits(again[k].double())), k
    with pytest.raises(ValueError, match='ws_cap'):
        ops.omlsa_rows(X, lengths=lens, ws_cap=per_row - 8)
    y = ops.omlsa_rows(X, lengths=lens, out_dtype=torch.float64)
    assert torch.equal(_bits(y), _bits(got['y']))
    assert torch.equal(_bits(baselines.omlsa(X.double(), 16000, lens)), _bits(y))


def test_output_dtypes_round_once(rows):
    from segan_pytorch_amd import ops
    names, X, lens = _ragged(rows)
    y64 = ops.omlsa_rows(X, lengths=lens, out_dtype=torch.float64)
    y32 = ops.omlsa_rows(X, lengths=lens)
    assert y32.dtype == torch.float32 and y64.dtype == torch.float64
    assert torch.equal(_bits(y32), _bits(y64.float()))
    # an fp64 input of the same values gives the same bits; its default output is fp64
    d64 = ops.omlsa_rows(X.double(), lengths=lens)
    assert d64.dtype == torch.float64 and torch.equal(_bits(d64), _bits(y64))
    d32 = ops.omlsa_rows(X.double(), lengths=lens, out_dtype=torch.float32)
    assert torch.equal(_bits(d32), _bits(y32))
    x8 = _cuda(rows['rate8'][0])
    a = ops.omlsa_rows(x8, srate=8000, out_dtype=torch.float64)
    assert torch.equal(_bits(ops.omlsa_rows(x8, srate=8000)), _bits(a.float()))


def test_omlsa_beats_both_rules_where_the_noise_level_changes(ofx, rows):
    from segan_pytorch_amd import baselines
    clean = ofx['signals']['clean4'].numpy()
    _, active = GO.gated6()
    X = _cuda(np.stack([rows[k][0] for k in CHANGING]))
    snr = {name: [GO.late_snr(clean, y, active) for y in fn(X).cpu().numpy()]
           for name, fn in (('noisy', lambda x: x), ('wiener', baselines.wiener),
                            ('logmmse', baselines.logmmse), ('omlsa', baselines.omlsa))}
    for i, kind in enumerate(CHANGING):
        print('{:9s} noisy {:.2f} dB: wiener {:.2f}, logmmse {:.2f}, omlsa {:.2f}'.format(
            kind, *(snr[k][i] for k in ('noisy', 'wiener', 'logmmse', 'omlsa'))))
        assert snr['omlsa'][i] > snr['wiener'][i] and snr['omlsa'][i] > snr['logmmse'][i], kind
        # fp32 output of the device against the oracle's figure in the fixture
        assert abs(snr['omlsa'][i] - ofx['meta']['late_snr'][kind]['omlsa']) < 1e-3


def test_validation_errors():
    from segan_pytorch_amd import baselines, ops
    x = torch.randn(2, 5000, device='cuda')
    for fn in (ops.omlsa_rows, ops.omlsa_stages):
        with pytest.raises(TypeError):
            fn(x.half())
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x.cpu())
        with pytest.raises(ValueError, match='srate'):
            fn(x, srate=44100)
        with pytest.raises(ValueError, match='lengths'):
            fn(x, lengths=[5000, 5001])
    with pytest.raises(RuntimeError, match='MI355X'):
        baselines.omlsa(x.cpu())
    short = x[:, :1000].contiguous()
    st = ops.omlsa_stages(short)                  # no row has a frame: everything is copied
    assert st['nframes'].tolist() == [0, 0] and st['presence'].shape == (2, 0)
    assert st['rough'].shape == (2, 0) and torch.isnan(st['noise']).all()
    assert torch.equal(st['y'], short)


def _run(args):
    p = subprocess.run(['timeout', '-k', '10', '120', sys.executable] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=ROOT,
                       universal_newlines=True)
    assert p.returncode == 0, p.stdout
    return p.stdout


def test_clean_cli_omlsa_writes_the_inputs_dtype_rate_and_length(ofx, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import baselines
    src, dst = tmp_path / 'in', tmp_path / 'out'
    src.mkdir()
    dst.mkdir()
    f16 = ofx['signals']['noisy'].numpy()[:12000]
    i16 = np.clip(np.rint(ofx['signals']['noisy'].numpy()[8000:24000].astype(np.float64) *
                          32768 * 4), -32768, 32767).astype(np.int16)
    wavfile.write(str(src / 'a.wav'), 16000, f16)
    wavfile.write(str(src / 'b.wav'), 16000, i16)
    out = _run([os.path.join(ROOT, 'clean.py'), '--omlsa', '--test_files', str(src),
                '--synthesis_path', str(dst), '--cuda'])
    assert 'Cleaning 2 wavs' in out
    rate, a = wavfile.read(str(dst / 'a.wav'))
    assert rate == 16000 and a.dtype == np.float32 and a.shape == f16.shape
    assert np.array_equal(a, baselines.omlsa(_cuda(f16)).cpu().numpy())
    assert np.array_equal(a, baselines.omlsa_wav(f16))
    rate, b = wavfile.read(str(dst / 'b.wav'))
    assert rate == 16000 and b.dtype == np.int16 and b.shape == i16.shape
    y = baselines.omlsa(_cuda(i16.astype(np.float32) / 32768).double()).cpu().numpy()
    assert np.array_equal(b, np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16))
    assert np.abs(b.astype(np.float64)).max() > 100 and not np.array_equal(b, i16)


def test_eval_cli_omlsa_measures_the_enhanced_signal(ofx, rows, tmp_path):
    from scipy.io import wavfile
    from segan_pytorch_amd import baselines
    from segan_pytorch_amd.quality import composite_eval
    cdir, ndir = tmp_path / 'clean', tmp_path / 'noisy'
    cdir.mkdir()
    ndir.mkdir()
    clean, noisy = ofx['signals']['clean4'].numpy(), rows['flat'][0]
    want = {}
    for name, L in (('a.wav', 32000), ('b.wav', 20000)):
        wavfile.write(str(cdir / name), 16000, clean[:L])
        wavfile.write(str(ndir / name), 16000, noisy[:L])
        enh = baselines.omlsa(_cuda(noisy[:L]))
        assert enh.dtype == torch.float32
        r = composite_eval(_cuda(clean[:L]), enh)
        plain = composite_eval(_cuda(clean[:L]), _cuda(noisy[:L]))
        want[name] = float(r['ssnr'][0])
        assert want[name] > float(plain['ssnr'][0])
    log = tmp_path / 'eval.log'
    _run([os.path.join(ROOT, 'eval_noisy_performance.py'), '--test_wavs', str(ndir),
          '--clean_wavs', str(cdir), '--logfile', str(log), '--omlsa'])
    lines = log.read_text().splitlines()
    assert lines[0] == 'FILE CSIG CBAK COVL PESQ SSNR'
    assert [l.split()[0] for l in lines[1:]] == ['a.wav', 'b.wav']
    for line in lines[1:]:
        f = line.split()
        assert len(f) == 6 and f[5] == '{:.3}'.format(want[f[0]]), line
