"""ops.resample on the MI355X against the fp64 oracle's fixture (tests/golden/resample.pt, written by
scripts/make_golden_resample.py), and the entry points that convert rates with it.

Every case is one ragged batch (rows of 0, 1 and 2 samples, one shorter than the filter, the rows
around the kernel's output tile, one of more than three tiles) converted once per dtype pair and
shared by the tests.  Bars: fp32 -> fp64 within 1e-12 of the oracle row's peak (the tolerance of
the STOI stage test for the same arithmetic: fp64 sums of at most 2 zeros max(p, q) / p + 1 <= 194
products here, fused multiply-adds on the device against separate roundings in numpy); fp32 output
bitwise the fp64 output rounded once; int16 exactly (the fixture keeps every expectation 1e-6 from
a half-integer); lengths and saturation counts exactly."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_resample as G  # noqa: E402
import resample_oracle as R  # noqa: E402

CASES = G.cases()
_RUNS = {}


def _id(case):
    return '{}to{}-z{}'.format(*case[:3])


@pytest.fixture(scope='module')
def rfx():
    return load_golden('resample.pt')


def _split(flat, out_lens):
    return list(torch.split(flat, out_lens))


def run(rfx, case):
    """The case's batch on the device, once: fp32 -> fp64, fp32 -> fp32, int16 -> int16."""
    if case not in _RUNS:
        from segan_pytorch_amd import ops
        a, b, zeros, beta = case
        e = rfx['cases'][case]
        lens, xf, xi, sq = G.case_inputs(case, e['seed'])
        assert lens == e['lens']
        xf_d, xi_d = torch.from_numpy(xf).cuda(), torch.from_numpy(xi).cuda()
        kw = dict(lengths=lens, zeros=zeros, beta=beta)
        _RUNS[case] = dict(
            lens=lens, xf=xf_d, xi=xi_d, sq=sq, e=e,
            f64=ops.resample(xf_d, a, b, out_dtype=torch.float64, **kw),
            f32=ops.resample(xf_d, a, b, **kw),
            i16=ops.resample(xi_d, a, b, **kw))
        torch.cuda.synchronize()
    return _RUNS[case]


def test_the_fixture_is_cut_for_this_kernels_tile(rfx):
    from segan_pytorch_amd import ops
    assert ops.resample_dims(1000, 48000, 16000) == (334, rfx['tile'])


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_fp64_output_lengths_and_padding(rfx, case):
    r = run(rfx, case)
    e = r['e']
    y, info = r['f64']
    assert y.dtype == torch.float64 and y.shape == (len(r['lens']), max(e['out_lens']))
    assert info['lengths'].dtype == torch.int32 and info['lengths'].tolist() == e['out_lens']
    assert info['nclip'].tolist() == [0] * len(r['lens'])
    y = y.cpu()
    for k, (want, Ly) in enumerate(zip(_split(e['y64'], e['out_lens']), e['out_lens'])):
        assert torch.count_nonzero(y[k, Ly:]) == 0, (case, k)
        if Ly:
            err = (y[k, :Ly] - want).abs().max().item()
            peak = want.abs().max().item()
            print(case, 'row of', r['lens'][k], 'samples: err / peak = {:.2e}'.format(err / peak))
            assert err <= 1e-12 * peak, (case, k, err, peak)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_fp32_output_is_the_fp64_output_rounded_once(rfx, case):
    r = run(rfx, case)
    y32, info = r['f32']
    assert y32.dtype == torch.float32 and info['lengths'].tolist() == r['e']['out_lens']
    assert torch.equal(y32, r['f64'][0].to(torch.float32))
    assert torch.equal(y32.view(torch.int32), r['f64'][0].to(torch.float32).view(torch.int32))


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_int16_to_int16_is_exact(rfx, case):
    r = run(rfx, case)
    e = r['e']
    y, info = r['i16']
    assert y.dtype == torch.int16 and y.shape == (len(r['lens']), max(e['out_lens']))
    assert info['lengths'].tolist() == e['out_lens']
    assert info['nclip'].tolist() == [0] * len(r['lens'])
    y = y.cpu()
    for k, (want, Ly) in enumerate(zip(_split(e['y16'], e['out_lens']), e['out_lens'])):
        assert torch.equal(y[k, :Ly], want), (case, k, (y[k, :Ly] != want).sum().item())
        assert torch.count_nonzero(y[k, Ly:]) == 0, (case, k)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_a_row_does_not_depend_on_the_batch_or_its_position(rfx, case):
    """Rows alone (T = their own length) and in the reversed batch are bitwise the rows of the
    batch, for the fp64 and the int16 path."""
    from segan_pytorch_amd import ops
    r = run(rfx, case)
    a, b, zeros, beta = case
    lens, outs = r['lens'], r['e']['out_lens']
    rows = len(lens)
    rev = list(range(rows - 1, -1, -1))
    rev_d = torch.tensor(rev, device='cuda')
    for x, key, dt in ((r['xf'], 'f64', torch.float64), (r['xi'], 'i16', None)):
        base = r[key][0]
        y, info = ops.resample(x[rev_d].contiguous(), a, b, lengths=[lens[k] for k in rev],
                               out_dtype=dt, zeros=zeros, beta=beta)
        assert info['lengths'].tolist() == [outs[k] for k in rev]
        assert torch.equal(y[rev_d], base), (case, key)
        for k in (rows - 1, rows - 2, 1):
            y1, i1 = ops.resample(x[k:k + 1, :lens[k]].contiguous(), a, b, out_dtype=dt, zeros=zeros,
                                  beta=beta)
            assert i1['lengths'].tolist() == [outs[k]] and y1.shape == (1, outs[k])
            assert torch.equal(y1[0], base[k, :outs[k]]), (case, key, k)


@pytest.mark.parametrize('case', CASES, ids=_id)
def test_a_full_scale_square_wave_saturates_and_is_counted(rfx, case):
    from segan_pytorch_amd import ops
    r = run(rfx, case)
    a, b, zeros, beta = case
    e = r['e']
    T = len(r['sq'])
    x = torch.stack([torch.from_numpy(r['sq']), r['xi'][-1].cpu(), torch.from_numpy(r['sq'])]).cuda()
    half = T // 2
    y, info = ops.resample(x, a, b, lengths=[T, r['lens'][-1], half], zeros=zeros, beta=beta)
    want = e['sq16']
    assert e['sq_peak'] > 36000 and e['sq_nclip'] > 0
    assert y.dtype == torch.int16 and torch.equal(y[0].cpu(), want)
    assert int(y.max()) == 32767 and int(y.min()) == -32768            # saturated, never wrapped
    half16, half_clip = R.convert_int16(r['sq'][:half], a, b, zeros, beta)
    assert R.half_distance(R.convert(r['sq'][:half], a, b, zeros, beta)) >= G.HALF_MARGIN
    assert np.array_equal(y[2, :len(half16)].cpu().numpy(), half16)
    assert torch.count_nonzero(y[2, len(half16):]) == 0
    assert info['nclip'].tolist() == [e['sq_nclip'], 0, half_clip]
    # other outputs saturate nothing and report no count
    y64, i64 = ops.resample(x, a, b, out_dtype=torch.float64, zeros=zeros, beta=beta)
    assert i64['nclip'].tolist() == [0, 0, 0]
    assert abs(y64[0].abs().max().item() - e['sq_peak']) <= 1e-12 * e['sq_peak']


@pytest.mark.parametrize('case', [CASES[0], CASES[3], CASES[11]], ids=_id)
def test_every_input_dtype_meets_every_output_dtype(rfx, case):
    from segan_pytorch_amd import ops
    r = run(rfx, case)
    a, b, zeros, beta = case
    kw = dict(lengths=r['lens'], zeros=zeros, beta=beta)
    i64, _ = ops.resample(r['xi'], a, b, out_dtype=torch.float64, **kw)
    i32, _ = ops.resample(r['xi'], a, b, out_dtype=torch.float32, **kw)
    assert torch.equal(i32, i64.to(torch.float32))
    assert torch.equal(torch.round(i64).to(torch.int16), r['i16'][0])      # no saturation here
    f16, info = ops.resample(r['xf'], a, b, out_dtype=torch.int16, **kw)
    want = torch.round(r['f64'][0])          # torch.round is half to even; |values| < 10
    assert torch.equal(f16, want.to(torch.int16)) and info['nclip'].tolist() == [0] * len(r['lens'])


def test_lengths_on_the_device_are_clamped_and_nothing_is_copied_back(rfx):
    from segan_pytorch_amd import ops
    case = CASES[0]
    r = run(rfx, case)
    a, b, zeros, beta = case
    rows, T = r['xf'].shape
    lens_d = torch.tensor(r['lens'], dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter('always')
        torch.cuda.set_sync_debug_mode('warn')
        try:
            y, info = ops.resample(r['xf'], a, b, lengths=lens_d, out_dtype=torch.float64, zeros=zeros,
                                   beta=beta)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert not [w for w in seen if 'called a synchronizing' in str(w.message).lower()], [str(w.message) for w in seen]
    assert torch.equal(y, r['f64'][0]) and torch.equal(info['lengths'], r['f64'][1]['lengths'])
    wild = lens_d.clone()
    wild[0], wild[-1] = -7, T + 1000
    y2, info2 = ops.resample(r['xf'], a, b, lengths=wild, out_dtype=torch.float64, zeros=zeros, beta=beta)
    assert torch.equal(y2, y) and torch.equal(info2['lengths'], info['lengths'])
    y3, info3 = ops.resample(r['xf'], a, b, out_dtype=torch.float64, zeros=zeros, beta=beta)   # all T
    assert info3['lengths'].tolist() == [max(r['e']['out_lens'])] * rows
    assert torch.equal(y3[-1], y[-1])
    with pytest.raises(ValueError, match='int32'):
        ops.resample(r['xf'], a, b, lengths=lens_d.to(torch.int64))


def test_equal_rates_copy_and_defaults_are_32_and_8_6(rfx):
    from segan_pytorch_amd import ops
    r = run(rfx, CASES[0])
    y, info = ops.resample(r['xi'], 16000, 16000, lengths=r['lens'])
    assert torch.equal(y, r['xi']) and info['lengths'].tolist() == r['lens']
    y, _ = ops.resample(r['xf'], 22050, 22050)
    assert torch.equal(y, r['xf'])
    y, _ = ops.resample(r['xi'], 48000, 16000, lengths=r['lens'])
    assert torch.equal(y, r['i16'][0])


# ------------------------------------------------------------------------------------------
# entry points
# ------------------------------------------------------------------------------------------
def _noise16(rng, n, amp=3000):
    return (rng.standard_normal(n) * amp).astype(np.int16)


def _oracle16(x, rate_in, rate_out=16000):
    y = R.convert(x, rate_in, rate_out)
    assert R.half_distance(y) >= G.HALF_MARGIN
    y16, nclip = R.to_int16(y)
    assert nclip == 0
    return y16


def _run(cmd):
    out = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-2000:]
    return out


def test_host_helpers_convert_like_the_oracle():
    from segan_pytorch_amd import resample
    rng = np.random.default_rng(5)
    mono48, mono44 = _noise16(rng, 5000), _noise16(rng, 3000)
    stereo48 = np.stack([_noise16(rng, 2000), _noise16(rng, 2000)], axis=1)
    flt32k = rng.standard_normal(1500)
    at16 = _noise16(rng, 700)
    y = resample.resample_wav(mono48, 48000)
    assert y.dtype == np.int16 and np.array_equal(y, _oracle16(mono48, 48000))
    outs, nclip = resample.resample_many([mono48, at16, stereo48, mono44, flt32k],
                                         [48000, 16000, 48000, 44100, 32000], max_batch_samples=6000)
    assert nclip == 0 and outs[1] is at16
    assert np.array_equal(outs[0], y)
    assert np.array_equal(outs[3], _oracle16(mono44, 44100))
    mean = stereo48.mean(axis=1, dtype=np.float32)
    assert outs[2].dtype == np.float32        # averaged channels are no int16 any more
    want = R.convert(mean, 48000, 16000)
    assert np.abs(outs[2] - want).max() <= 2.0 ** -23 * np.abs(want).max()      # one fp32 rounding
    assert outs[4].dtype == np.float32
    want = R.convert(flt32k.astype(np.float32), 32000, 16000)
    assert outs[4].shape == want.shape == (750,)
    assert np.abs(outs[4] - want).max() <= 2.0 ** -23 * np.abs(want).max()
    loud = np.where((np.arange(4000) // 40) % 2 == 0, 32767, -32768).astype(np.int16)
    assert R.half_distance(R.convert(loud, 48000, 16000)) >= G.HALF_MARGIN
    y16, n = R.convert_int16(loud, 48000, 16000)
    outs, nclip = resample.resample_many([loud], 48000)
    assert np.array_equal(outs[0], y16) and nclip == n > 0


def test_noise_bank_from_dir_holds_the_converted_noises(tmp_path):
    from segan_pytorch_amd.augment import NoiseBank
    rng = np.random.default_rng(6)
    n48, n44, n16 = _noise16(rng, 6000), _noise16(rng, 4410), _noise16(rng, 900)
    wavfile.write(str(tmp_path / 'a48.wav'), 48000, n48)
    wavfile.write(str(tmp_path / 'b44.wav'), 44100, n44)
    wavfile.write(str(tmp_path / 'c16.wav'), 16000, n16)
    bank = NoiseBank.from_dir(str(tmp_path), target_rate=16000)
    want = [_oracle16(n48, 48000), _oracle16(n44, 44100), n16]
    assert bank.lengths.tolist() == [len(w) for w in want] == [2000, 1600, 900]
    assert np.array_equal(bank.host, np.concatenate(want).astype(np.float32) / np.float32(32768))
    plain = NoiseBank.from_dir(str(tmp_path))           # without it the rate is ignored, as before
    assert plain.lengths.tolist() == [6000, 4410, 900]


def _pairs(tmp_path, rng, rate, n, names=('u0', 'u1')):
    """clean / noisy int16 wav pairs at `rate` and their oracle-converted 16 kHz copies."""
    dirs = {k: tmp_path / k for k in ('clean', 'noisy', 'clean16', 'noisy16')}
    for d in dirs.values():
        d.mkdir()
    for name in names:
        c = _noise16(rng, n, 4000)
        x = (c + rng.standard_normal(n) * 500).astype(np.int16)
        for k, w in (('clean', c), ('noisy', x)):
            wavfile.write(str(dirs[k] / (name + '.wav')), rate, w)
            wavfile.write(str(dirs[k + '16'] / (name + '.wav')), 16000, _oracle16(w, rate))
    return {k: str(v) for k, v in dirs.items()}


def test_make_pcm_shard_resample_equals_the_shard_of_the_converted_files(tmp_path):
    d = _pairs(tmp_path, np.random.default_rng(7), 48000, 7000)
    tool = os.path.join(ROOT, 'scripts', 'make_pcm_shard.py')
    _run([tool, d['clean'], d['noisy'], str(tmp_path / 'r'), '--slice_size', '1024', '--resample'])
    _run([tool, d['clean16'], d['noisy16'], str(tmp_path / 'p'), '--slice_size', '1024'])
    got, want = (tmp_path / 'r.pcm16').read_bytes(), (tmp_path / 'p.pcm16').read_bytes()
    assert len(want) >= 4 * 2 * 1025 * 2 and got == want
    assert (tmp_path / 'r.json').read_bytes() == (tmp_path / 'p.json').read_bytes()


def test_eval_cli_resample_equals_the_run_on_converted_copies(tmp_path):
    d = _pairs(tmp_path, np.random.default_rng(8), 48000, 30000)
    tool = os.path.join(ROOT, 'eval_noisy_performance.py')
    _run([tool, '--test_wavs', d['noisy'], '--clean_wavs', d['clean'], '--logfile',
          str(tmp_path / 'r.log'), '--stoi', '--resample'])
    _run([tool, '--test_wavs', d['noisy16'], '--clean_wavs', d['clean16'], '--logfile',
          str(tmp_path / 'p.log'), '--stoi'])
    got, want = (tmp_path / 'r.log').read_text(), (tmp_path / 'p.log').read_text()
    assert len(want.splitlines()) == 3 and got == want


@pytest.fixture(scope='module')
def cleaned(tmp_path_factory):
    """A tiny generator (train.py, synthetic data), a 48 kHz wav, the 16 kHz int16 wav the oracle makes
    of it and clean.py's output for that one (same seed and generator as tests/test_gpu_cli.py)."""
    tmp = tmp_path_factory.mktemp('clean_resample')
    ck = str(tmp / 'ckpt')
    _run([os.path.join(ROOT, 'train.py'), '--save_path', ck, '--synthetic', '8', '--batch_size', '4',
          '--epoch', '1', '--save_freq', '1', '--no_train_gen', '--genc_fmaps', '8', '16', '32',
          '--denc_fmaps', '8', '16', '32', '--genc_poolings', '4', '4', '4', '--denc_poolings', '4',
          '4', '4', '--z_dim', '32', '--slice_size', '1024', '--num_workers', '0'])
    g_ckpt = [n for n in os.listdir(ck) if n.startswith('weights_EOE_G-Generator-')][0]
    x48 = _noise16(np.random.default_rng(9), 10001)
    d48, d16 = tmp / 'in48', tmp / 'in16'
    d48.mkdir()
    d16.mkdir()
    wavfile.write(str(d48 / 'a.wav'), 48000, x48)
    wavfile.write(str(d16 / 'a.wav'), 16000, _oracle16(x48, 48000))
    base = [os.path.join(ROOT, 'clean.py'), '--g_pretrained_ckpt', os.path.join(ck, g_ckpt),
            '--cfg_file', os.path.join(ck, 'train.opts'), '--cuda']
    _run(base + ['--test_files', str(d16), '--synthesis_path', str(tmp / 'o_16')])
    return dict(tmp=tmp, base=base, d48=str(d48), out16=tmp / 'o_16' / 'a.wav')


def test_clean_cli_resample_equals_clean_on_the_converted_wav(cleaned):
    """clean.py --resample on a 48 kHz wav writes the bytes clean.py writes for the 16 kHz int16 wav
    the oracle makes of it."""
    out = cleaned['tmp'] / 'o_res'
    _run(cleaned['base'] + ['--test_files', cleaned['d48'], '--synthesis_path', str(out), '--resample'])
    assert (out / 'a.wav').read_bytes() == cleaned['out16'].read_bytes()
    rate, enh = wavfile.read(str(out / 'a.wav'))
    assert rate == 16000 and enh.shape == (3334,) and enh.dtype == np.float32


def test_clean_cli_keep_rate_writes_the_inputs_rate_and_length(cleaned):
    out = cleaned['tmp'] / 'o_keep'
    _run(cleaned['base'] + ['--test_files', cleaned['d48'], '--synthesis_path', str(out), '--keep_rate'])
    rate, kept = wavfile.read(str(out / 'a.wav'))
    assert rate == 48000 and kept.shape == (10001,) and kept.dtype == np.float32
    assert np.isfinite(kept).all()
    # it is the 16 kHz result converted back: the oracle's conversion of it, rounded to fp32
    back = R.convert(wavfile.read(str(cleaned['out16']))[1], 16000, 48000)[:10001]
    assert np.abs(kept - back).max() <= 2.0 ** -23 * np.abs(back).max()      # one fp32 rounding
