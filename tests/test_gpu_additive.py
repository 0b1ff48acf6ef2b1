"""The additive-noise mixer on the MI355X (ops.asl_p56 / ops.additive_mix, augment.Additive,
PCMShardLoader's mixer, train.py --additive_noises) against the real reference's results
(tests/golden/additive.pt, recipe scripts/make_golden_additive.py).

Bounds.  The envelope q is compared peak-relative at 1e-12 (the criterion of the fp64 filter
stages in test_gpu_stoi.py).  The counts are exact: the fixture keeps every q[k] more than 1e-9
(relative) away from every threshold.  asl_ms, asl, c0, sq, Pn and sf were measured against the
all-float64 run of the reference: the largest relative deviation over the ten cases is 5.9e-16
(asl_ms of `clip`); the bound is 100 x that rounded up to a power of ten, 1e-13.  noisy: within
one fp32 ulp of the float64 truth rounded to fp32, and its largest error against the float64 truth
no larger than that of the reference's own literal float32-dot run (or one ulp of 1.0 where that is
larger)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import additive_oracle as A  # noqa: E402
import make_golden_additive as G  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ('ord16k', 'ord40k', 'quiet', 'low', 'zeros', 'zero_run', 'extreme', 'clip', 'short', 'sr8k')
TOL = 1e-13          # see the module docstring
ULP1 = 2.0 ** -24    # one fp32 ulp just below 1.0: the outputs lie in [-1, 1)


@pytest.fixture(scope='module')
def afx():
    return load_golden('additive.pt')


@pytest.fixture(scope='module')
def noises():
    return G.noise_bank()


@pytest.fixture(scope='module')
def bank(noises):
    from segan_pytorch_amd.augment import NoiseBank
    return NoiseBank(noises)


@pytest.fixture(scope='module')
def signals(afx):
    return {k: G.case_signal(rc) for k, rc in afx['cases'].items()}


def _rel(got, want):
    return abs(got - want) / abs(want) if want != 0 else abs(got)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _row(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda().unsqueeze(0)


@pytest.mark.parametrize('name', CASES)
def test_level_and_mix_match_the_reference(afx, noises, bank, signals, name):
    from segan_pytorch_amd import ops
    rc, t, lit = afx['cases'][name], afx['truth'][name], afx['literal'][name]
    x = signals[name]
    st = ops.asl_p56_stages(_row(x), rc['srate'])
    q = A.envelope(x, rc['srate'])
    qerr = np.abs(st['q'][0].cpu().numpy() - q).max()
    print(name, 'q peak-relative', qerr / max(q.max(), 1e-300))
    assert qerr <= 1e-12 * q.max()
    if name in afx['q']:
        want = afx['q'][name].numpy()
        assert np.abs(st['q'][0].cpu().numpy() - want).max() <= 1e-12 * want.max()
    assert st['counts'][0].cpu().tolist() == t['counts'].tolist()
    assert int(st['status'][0]) == 0
    for k in ('sq', 'asl_ms', 'asl'):
        print(name, k, _rel(float(st[k][0]), t[k]))
        assert _rel(float(st[k][0]), t[k]) <= TOL, k
    c0 = float(st['c0'][0])
    if math.isnan(t['c0']):      # the reference returns (0, 0, None)
        assert math.isnan(c0) and float(st['asl_ms'][0]) == 0.0 and float(st['asl'][0]) == 0.0
    else:
        print(name, 'c0', _rel(c0, t['c0']))
        assert _rel(c0, t['c0']) <= TOL

    ab = int(bank.offsets[t['noise_idx']]) + t['start']
    noisy, info = ops.additive_mix(_row(x), bank.data('cuda'), [ab], [t['snr']], st['asl_ms'])
    for k in ('Pn', 'sf'):
        print(name, k, _rel(float(info[k][0]), t[k]))
        assert _rel(float(info[k][0]), t[k]) <= TOL, k
    assert int(info['n'][0]) == t['n'] and int(info['status'][0]) == 0
    seg = noises[t['noise_idx']][t['start']:t['start'] + rc['T']]
    t64 = G.truth_mix(x, seg, t['sf'], t['n'])
    t32 = t64.astype(np.float32)
    assert G.sha(t32) == afx['sha'][name]['noisy32']      # the reference's own output
    got = noisy[0].cpu().numpy()
    err = np.abs(got.astype(np.float64) - t64).max()
    print(name, 'ulps', _ulps(got, t32).max(), 'err', err, 'literal', lit['err'])
    assert _ulps(got, t32).max() <= 1
    assert err <= max(lit['err'], ULP1)
    assert got.max() < 1.0 and got.min() >= -1.0
    if t['asl_ms'] == 0:      # Px == 0: sf = 0, noisy == clean bit for bit
        assert float(info['sf'][0]) == 0.0 and np.array_equal(got, x)
    else:                     # the achieved SNR is the requested one
        sf, Pn = float(info['sf'][0]), float(info['Pn'][0])
        assert abs(10 * math.log10(float(st['asl_ms'][0]) / (sf * sf * Pn)) - t['snr']) <= 1e-9
    if name == 'clip':
        assert t['n'] >= 1 and np.abs(G.truth_mix(x, seg, t['sf'], 0)).max() >= 1.0


def test_a_row_longer_than_2_to_the_20(bank):
    """T = 2^20 + 3 (512 slabs and a tail of three samples) against the numpy oracle."""
    from segan_pytorch_amd import ops
    T = (1 << 20) + 3
    x = G.speech_like(T, 16000, 77)
    o = A.asl_p56(x)
    assert A.threshold_margin(o['q']) > 1e-9 and o['c0'] is not None
    st = ops.asl_p56_stages(_row(x))
    assert np.abs(st['q'][0].cpu().numpy() - o['q']).max() <= 1e-12 * o['q'].max()
    assert st['counts'][0].cpu().tolist() == o['counts'].tolist()
    for k in ('sq', 'asl_ms', 'asl', 'c0'):
        assert _rel(float(st[k][0]), o[k]) <= TOL, k
    small = NoiseBankOf(T + 10)
    noisy, info = ops.additive_mix(_row(x), small, [7], [5], st['asl_ms'])
    m = A.mix(x, small[7:7 + T].cpu().numpy(), 5, o['asl_ms'])
    assert int(info['n'][0]) == m['n'] and _rel(float(info['sf'][0]), m['sf']) <= TOL
    assert _ulps(noisy[0].cpu().numpy(), m['noisy32']).max() <= 1


def NoiseBankOf(n):
    return torch.from_numpy((0.05 * np.random.default_rng(8).standard_normal(n)).astype(np.float32)).cuda()


def test_batched_rows_with_lengths_equal_single_rows(afx, noises, bank, signals):
    """Rows of different lengths in one launch, in two orders: every row's results are those of
    the row run alone (bit for bit), whatever its position; q is zero and noisy is clean past the
    row's length."""
    from segan_pytorch_amd import ops
    names = ('ord16k', 'short', 'clip', 'zeros', 'extreme', 'sr8k')
    lens = [len(signals[n]) for n in names]
    T = max(lens) + 5
    X = np.zeros((len(names), T), np.float32)
    for r, n in enumerate(names):
        X[r, :lens[r]] = signals[n]
        X[r, lens[r]:] = 0.25      # must not be read
    starts = [int(bank.offsets[afx['truth'][n]['noise_idx']]) + afx['truth'][n]['start'] for n in names]
    snrs = [afx['truth'][n]['snr'] for n in names]
    single = []
    for r, n in enumerate(names):
        xr = _row(signals[n])
        lv = ops.asl_p56_stages(xr, 16000)
        ny, info = ops.additive_mix(xr, bank.data('cuda'), [starts[r]], [snrs[r]], lv['asl_ms'])
        single.append((lv, ny, info))
    for order in (list(range(len(names))), [3, 5, 0, 2, 4, 1]):
        Xd = torch.from_numpy(X[order]).cuda()
        ln = [lens[i] for i in order]
        lv = ops.asl_p56_stages(Xd, 16000, lengths=ln)
        ny, info = ops.additive_mix(Xd, bank.data('cuda'), [starts[i] for i in order],
                                    [snrs[i] for i in order], lv['asl_ms'], lengths=ln)
        for r, i in enumerate(order):
            slv, sny, sinfo = single[i]
            for k in ('sq', 'asl_ms', 'asl', 'c0'):
                assert torch.equal(lv[k][r:r + 1].view(torch.int64), slv[k].view(torch.int64)), k
            assert torch.equal(lv['counts'][r], slv['counts'][0])
            assert torch.equal(lv['q'][r, :ln[r]], slv['q'][0])
            assert not lv['q'][r, ln[r]:].any()
            for k in ('Pn', 'sf'):
                assert torch.equal(info[k][r:r + 1].view(torch.int64), sinfo[k].view(torch.int64)), k
            assert int(info['n'][r]) == int(sinfo['n'][0])
            assert torch.equal(ny[r, :ln[r]], sny[0])
            assert torch.equal(ny[r, ln[r]:], Xd[r, ln[r]:])
    assert set(ops.asl_p56(Xd, 16000, lengths=ln)) == {'sq', 'asl_ms', 'asl', 'c0', 'counts', 'status'}


def test_arguments_are_checked_before_any_launch(bank):
    from segan_pytorch_amd import ops
    x = torch.zeros(2, 100, device='cuda')
    px = torch.ones(2, dtype=torch.float64, device='cuda')
    b = bank.data('cuda')
    n = b.numel()
    with pytest.raises(NotImplementedError, match='nbits'):
        ops.asl_p56(x, 16000, nbits=8)
    with pytest.raises(ValueError, match='srate'):
        ops.asl_p56(x, 0)
    with pytest.raises(ValueError, match='lengths'):
        ops.asl_p56(x, lengths=[100, 101])
    for starts in ([0, n - 99], [-1, 0], [0, n]):
        with pytest.raises(ValueError, match='outside the noise bank'):
            ops.additive_mix(x, b, starts, [0, 0], px)
    ops.additive_mix(x, b, [0, n - 100], [0, 0], px)      # the last valid start
    with pytest.raises(ValueError, match='outside the noise bank'):      # prev reads start - 1
        ops.additive_mix(x, b, [0, 5], [0, 0], px, prev=torch.zeros(2, device='cuda'))
    with pytest.raises(ValueError, match='snrs'):
        ops.additive_mix(x, b, [0, 0], [0, float('nan')], px)
    with pytest.raises(ValueError, match='starts must hold 2'):
        ops.additive_mix(x, b, [0], [0, 0], px)
    with pytest.raises(TypeError, match='px'):
        ops.additive_mix(x, b, [0, 0], [0, 0], px.float())
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.additive_mix(x, b.cpu(), [0, 0], [0, 0], px)


def test_silent_noise_segment_returns_clean_and_flags_it(signals):
    from segan_pytorch_amd import ops
    x = _row(signals['ord16k'])
    silent = torch.zeros(20000, device='cuda')
    lv = ops.asl_p56(x)
    noisy, info = ops.additive_mix(x, silent, [7], [5], lv['asl_ms'])
    assert torch.equal(noisy, x)
    assert int(info['status'][0]) == ops.ADDITIVE_PN0 and float(info['sf'][0]) == 0.0
    assert float(info['Pn'][0]) == 0.0 and int(info['n'][0]) == 0


def test_additive_object_mixes_like_the_reference(afx, noises, bank, signals):
    """Additive.mix with the reference's recorded draws reproduces the reference's output;
    __call__ returns a CPU FloatTensor of the waveform's length; draws repeat with the seed."""
    from segan_pytorch_amd.augment import Additive, ComposeAdditive
    add = Additive(bank, seed=5)
    for name in ('ord16k', 'clip'):
        t = afx['truth'][name]
        noisy, info = add.mix(_row(signals[name]), noise_ids=[t['noise_idx']], snrs=[t['snr']],
                              starts=[t['start']])
        assert G.sha(noisy[0].cpu().numpy()) == afx['sha'][name]['noisy32']
        assert info['abs_starts'].tolist() == [int(bank.offsets[t['noise_idx']]) + t['start']]
    wav = signals['ord40k'][:12345]
    a = Additive(bank, snr_levels=[0, 5, 10], seed=9)(wav)
    b = Additive(bank, snr_levels=[0, 5, 10], seed=9)(torch.from_numpy(wav).view(1, -1))
    c = Additive(bank, snr_levels=[0, 5, 10], seed=10)(wav)
    assert a.type() == 'torch.FloatTensor' and tuple(a.shape) == (12345,)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.max() < 1 and a.min() >= -1 and not torch.equal(a, torch.from_numpy(wav))
    x, y = ComposeAdditive(Additive(bank, seed=9))(wav)
    assert x is wav and torch.equal(y, a)
    with pytest.raises(ValueError, match='Noise length has to be greater than speech length'):
        Additive([np.ones(100, np.float32)])(wav)


# ---- the loader ---------------------------------------------------------------------------------

T_SLICE = 4096


@pytest.fixture(scope='module')
def shard(tmp_path_factory):
    """Three 16-bit utterances (speech-like, 2.4 .. 3 slices each) cut into 4096-sample slices."""
    from segan_pytorch_amd.datasets import PCMShardDataset, build_pcm_shard
    d = tmp_path_factory.mktemp('additive_shard')
    cd, nd = d / 'clean', d / 'noisy'
    cd.mkdir()
    nd.mkdir()
    rng = np.random.default_rng(21)
    for i, n in enumerate((10000, 12288, 9000)):
        c = np.rint(G.speech_like(n, 16000, 30 + i).astype(np.float64) * 40000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000,
                      (c + rng.standard_normal(n) * 300).astype(np.int16))
    assert build_pcm_shard(str(cd), str(nd), str(d / 'sh'), slice_size=T_SLICE, stride=0.5) >= 9
    return PCMShardDataset(str(d / 'sh'))


def _loader(shard, additive=None, **kw):
    from torch.utils.data import SequentialSampler
    from segan_pytorch_amd.datasets import PCMShardLoader
    return PCMShardLoader(shard, 4, 0.95, 'cuda', sampler=SequentialSampler(shard), num_workers=0,
                          additive=additive, record_additive=True, **kw)


def _batches(loader):
    out = [(list(n), c.cpu(), y.cpu(), i) for n, c, y, i in loader]
    return out, loader.additive_records


@pytest.fixture(scope='module')
def plain(shard):
    return _batches(_loader(shard))[0]


def test_loader_mix_is_the_composition_of_the_public_ops(shard, bank, plain):
    """Per slice: wave = fp32(min-max normalised clean slice); level, Pn and the clipping test over
    its T samples; the sample before the slice is (clean_prev + sf * noise[s-1]) after the same n
    divisions, rounded to fp32; pre-emphasis in double, rounded once; y[0] = x[0] where the slice
    starts its wav.  Composed here on the host in float64 from `info`."""
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import Additive
    got, recs = _batches(_loader(shard, Additive(bank, seed=1), additive_seed=111))
    assert len(got) == len(plain) == len(recs) and len(got) >= 3
    n_first = 0
    for k, ((names, clean, noisy, idx), (pn, pc, py, pi), info) in enumerate(zip(got, plain, recs)):
        assert torch.equal(clean, pc) and torch.equal(idx, pi)      # clean rows: bit-identical
        assert names == [n + '_additive' for n in pn]               # prob 1: every item
        sel = info['index']
        assert sel.tolist() == list(range(len(names)))
        items = list(range(len(names)))
        base = 4 * k
        pcm = np.stack([np.array(shard.data[base + r]) for r in items])
        first = shard._first[base:base + len(items)]
        wave = ((2.0 / 65535.0) * (pcm[:, 0].astype(np.float64) - 32767.0) + 1.0).astype(np.float32)
        assert np.array_equal(info['wave'].cpu().numpy(), wave[:, 1:])
        assert np.array_equal(info['wave_prev'].cpu().numpy(), wave[:, 0])
        lv = ops.asl_p56(torch.from_numpy(wave[:, 1:].copy()).cuda())
        assert torch.equal(lv['asl_ms'], info['asl_ms'])
        for r in items:
            ab, sf, n = int(info['abs_starts'][r]), float(info['sf'][r]), int(info['n'][r])
            assert info['starts'][r] >= 1
            o = A.asl_p56(wave[r, 1:])
            assert _rel(float(info['asl_ms'][r]), o['asl_ms']) <= TOL
            assert o['asl_ms'] > 0 and sf > 0
            m = A.mix(wave[r, 1:], bank.host[ab:ab + T_SLICE], info['snrs'][r], o['asl_ms'])
            assert m['n'] == n and _rel(sf, m['sf']) <= TOL
            v = G.truth_mix(wave[r], bank.host[ab - 1:ab + T_SLICE], sf, n).astype(np.float32)
            assert np.array_equal(info['mixed'][r].cpu().numpy(), v[1:])
            assert np.array_equal(info['prev'][r].cpu().numpy(), v[0])
            v = v.astype(np.float64)
            y = v[1:] - 0.95 * v[:-1]
            if first[r]:
                y[0] = v[1]
                n_first += 1
            assert np.array_equal(noisy[r].numpy(), y.astype(np.float32))
            assert not torch.equal(noisy[r], py[r])
    assert n_first == 3      # one slice per utterance starts its wav


def test_loader_probability_names_seeds_and_sample(shard, bank, plain):
    from segan_pytorch_amd.augment import Additive
    # prob 0: the unaugmented batches, bit for bit
    got, recs = _batches(_loader(shard, Additive(bank, seed=1), additive_prob=0.0, additive_seed=3))
    assert recs == [None] * len(plain)
    for a, b in zip(got, plain):
        assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # prob 0.5: '_additive' exactly on the mixed items, the others keep the shard's noisy row
    got, recs = _batches(_loader(shard, Additive(bank, seed=1), additive_prob=0.5, additive_seed=3))
    mixed = 0
    for (names, clean, noisy, _), (pn, pc, py, _), info in zip(got, plain, recs):
        sel = set() if info is None else set(info['index'].tolist())
        assert torch.equal(clean, pc)
        for r, name in enumerate(names):
            assert name == (pn[r] + '_additive' if r in sel else pn[r])
            assert torch.equal(noisy[r], py[r]) != (r in sel)
        mixed += len(sel)
    assert 0 < mixed < sum(len(b[0]) for b in plain)
    # the same seed repeats, another rank's seed draws another stream
    again, _ = _batches(_loader(shard, Additive(bank, seed=1), additive_prob=0.5, additive_seed=3))
    other, orec = _batches(_loader(shard, Additive(bank, seed=1), additive_prob=0.5, additive_seed=4))
    assert all(a[0] == b[0] and torch.equal(a[2], b[2]) for a, b in zip(got, again))
    assert any(a[0] != b[0] or not torch.equal(a[2], b[2]) for a, b in zip(got, other))
    # sample() (WSEGAN) goes through the same path
    ld = _loader(shard, Additive(bank, seed=1), additive_seed=5)
    names, clean, noisy, _ = ld.sample()
    assert all(n.endswith('_additive') for n in names) and len(ld.additive_records) >= 1
    assert noisy.is_cuda and bool(torch.isfinite(noisy).all())
    ld.close()


# ---- train.py -----------------------------------------------------------------------------------

@pytest.mark.parametrize('extra', [[], ['--wsegan', '--opt', 'adam']], ids=['segan', 'wsegan'])
def test_train_with_additive_noises(tmp_path, extra):
    from segan_pytorch_amd.datasets import build_pcm_shard
    rng = np.random.default_rng(2)
    cd, nd, zd = tmp_path / 'clean', tmp_path / 'noisy', tmp_path / 'noises'
    for d in (cd, nd, zd):
        d.mkdir()
    for i in range(3):
        c = np.rint(G.speech_like(6000, 16000, 40 + i).astype(np.float64) * 30000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000, c)
    for i in range(2):
        wavfile.write(str(zd / 'n{}.wav'.format(i)), 16000,
                      (rng.standard_normal(5000 + 1000 * i) * 2000).astype(np.int16))
    assert build_pcm_shard(str(cd), str(nd), str(tmp_path / 'sh'), slice_size=1024, stride=0.5) >= 8
    ck = str(tmp_path / 'ckpt')
    cmd = [sys.executable, os.path.join(ROOT, 'train.py'), '--save_path', ck, '--pcm_shard',
           str(tmp_path / 'sh'), '--additive_noises', str(zd), '--additive_snrs', '0', '10',
           '--additive_prob', '0.75', '--batch_size', '4', '--epoch', '1', '--save_freq', '1',
           '--no_train_gen', '--genc_fmaps', '8', '16', '32', '--denc_fmaps', '8', '16', '32',
           '--genc_poolings', '4', '4', '4', '--denc_poolings', '4', '4', '4', '--z_dim', '32',
           '--slice_size', '1024', '--num_workers', '0'] + extra
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'btime' in out.stdout and 'nan' not in out.stdout.lower()
    opts = json.load(open(os.path.join(ck, 'train.opts')))
    assert opts['additive_snrs'] == [0.0, 10.0] and opts['additive_prob'] == 0.75
    assert any(n.startswith('weights_EOE_G-Generator-') for n in os.listdir(ck))
