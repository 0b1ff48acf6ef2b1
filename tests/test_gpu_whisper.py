"""Whispered speech on the MI355X (ops.whisper_noise / whisper_stages / whisper_lpc / whisper_rows,
augment.Whisper, PCMShardLoader's whisper stage) against the float64 oracle
scripts/whisper_oracle.py on the cases of tests/golden/whisper.pt (recipe
scripts/make_golden_whisper.py).

Bounds.  The excitation is integer arithmetic and one division: bit-equal.  Lags, coefficients,
sigma, peak and the fp64 output are compared within 100 x the largest movement of that quantity
between the oracle's float64 and longdouble runs over the fixture's cases (the recipe records it;
the SRMR precedent), relative to the case's largest magnitude of that quantity: 1.8e-14 for the
lags, 2.4e-10 for a, 8.7e-11 for sigma, 2.5e-11 for y.  Status, silent frames and orders are equal.
The fp32 output is within one fp32 ulp of the rounded fp64 oracle.  Measured on an MI355X: see
DESIGN.md section 18."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_additive as GA  # noqa: E402
import make_golden_reverb as GR  # noqa: E402
import whisper_oracle as W  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 100.0


@pytest.fixture(scope='module')
def wfx():
    return load_golden('whisper.pt')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.cpu().numpy()


def _scalar(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32, device='cuda')


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _rel(got, want):
    want = np.asarray(want, dtype=np.float64)
    m = np.abs(want).max() if want.size else 0.0
    d = np.abs(np.asarray(got, dtype=np.float64) - want).max() if want.size else 0.0
    return d / m if m > 0 else d


def _ulps32(got, want64):
    """|got - float32(want64)| in units of the fp32 spacing at float32(want64)"""
    w32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(w32), np.float32(2.0 ** -126)))
    return float((np.abs(got.astype(np.float64) - w32.astype(np.float64)) / sp).max()) if w32.size \
        else 0.0


# ---- the excitation -------------------------------------------------------------------------------

@pytest.mark.parametrize('j0', [-513, 0, 2 ** 20 - 5])
@pytest.mark.parametrize('count', [1, 64, 769])
def test_noise_bit_equal(j0, count):
    from segan_pytorch_amd import ops
    seeds = [0, 2 ** 63 - 1]
    u = _np(ops.whisper_noise(seeds, j0, count))
    assert u.shape == (2, count) and u.dtype == np.float64
    for r, s in enumerate(seeds):
        assert _same(u[r], W.noise(s, j0, count)), (s, j0, count)
    ud = _np(ops.whisper_noise(_dev(np.asarray(seeds, dtype=np.int64)), j0, count))
    assert _same(u, ud)


# ---- the stages against the oracle ----------------------------------------------------------------

def _case_args(c):
    x = c['x'].cuda()[None].contiguous()
    lengths = None if c['length'] is None else [c['length']]
    return x, [c['seed']], [c['tilt']], lengths, _scalar(c['prev'])[None].contiguous()


CASES = ['one', 'short', 't255', 't256', 't257', 'odd', 'full', 'full_tilt', 'partial', 'len_hop',
         'empty_prev', 'empty', 'gap', 'zeros', 'guard', 'lag60']


@pytest.mark.parametrize('name', CASES)
def test_stages_and_rows_against_the_oracle(name, wfx):
    from segan_pytorch_amd import ops
    c, big = wfx['cases'][name], wfx['largest_move']
    x, seeds, tilts, lengths, prev = _case_args(c)
    T = x.shape[1]
    n = T if c['length'] is None else c['length']
    F = n // 256 + 2
    st = ops.whisper_stages(x, seeds, tilts, lengths, prev, lag_hz=c['lag_hz'])
    y32, info = ops.whisper_rows(x, seeds, tilts, lengths, prev, lag_hz=c['lag_hz'])
    y64, info64 = ops.whisper_rows(x, seeds, tilts, lengths, prev, out_dtype=torch.float64,
                                   lag_hz=c['lag_hz'])
    torch.cuda.synchronize()
    want_y = np.concatenate([[c['prev_out']], _np(c['out'])])
    got_y = np.concatenate([_np(st['prev64']), _np(st['y64'][0])])
    d = dict(r=_rel(_np(st['r'][0, :F]), _np(c['r'])), a=_rel(_np(st['a'][0, :F]), _np(c['a'])),
             sigma=_rel(_np(st['sigma'][0, :F]), _np(c['sigma'])), y=_rel(got_y, want_y),
             peak=_rel(_np(st['peak']), [c['peak']]))
    ulps = max(_ulps32(_np(y32[0]), _np(c['out'])), _ulps32(_np(info['prev']), [c['prev_out']]))
    print('whisper {:11s} distance r={:.2e} a={:.2e} sigma={:.2e} y={:.2e} peak={:.2e} fp32 ulps='
          '{:.2f}'.format(name, d['r'], d['a'], d['sigma'], d['y'], d['peak'], ulps))
    for res in (st, info, info64):
        assert int(res['status'][0]) == c['status']
        assert int(res['nsilent'][0]) == c['nsilent']
        assert int(res['minorder'][0]) == c['minorder']
    assert np.array_equal(_np(st['order'][0, :F]), _np(c['order']))
    assert (_np(st['r'][0, F:]) == 0).all()          # frames past the row's own see zeros only
    for k in ('r', 'a', 'sigma', 'y', 'peak'):
        assert d[k] <= SCALE * big[k], (k, d[k], SCALE * big[k])
    # the whole call is the stages' result; zero from len on (unchanged rows are copied)
    assert _same(_np(y64), _np(st['y64'])) and _same(_np(info64['prev']), _np(st['prev64']))
    assert _same(_np(info64['peak']), _np(st['peak'])) and _same(_np(info['peak']), _np(st['peak']))
    if c['status'] == 0:
        assert (_np(y64[0, n:]) == 0).all() and (_np(y32[0, n:]) == 0).all()
    else:
        assert _same(_np(y32), _np(x)) and _same(_np(info['prev']), _np(prev))
    assert ulps <= 1.0
    assert _same(_np(y32), _np(y64).astype(np.float32))          # rounded once from the fp64 result
    assert float(y32.abs().max()) <= 1.0


def test_peak_guard(wfx):
    from segan_pytorch_amd import ops
    c, big = wfx['cases']['guard'], wfx['largest_move']
    assert c['peak'] > 1.0 and abs(float(c['x'].abs().max()) - 0.9) < 1e-4
    x, seeds, tilts, lengths, prev = _case_args(c)
    y, info = ops.whisper_rows(x, seeds, tilts, lengths, prev)
    assert abs(float(info['peak'][0]) - c['peak']) <= SCALE * big['peak'] * c['peak']
    assert float(y.abs().max()) <= 1.0 and float(info['prev'].abs().max()) <= 1.0
    y64, _ = ops.whisper_rows(x, seeds, tilts, lengths, prev, out_dtype=torch.float64)
    assert float(y64.abs().max()) == 1.0


def test_lpc_guards_on_crafted_lags():
    from segan_pytorch_amd import ops
    r = np.zeros((5, 17))
    r[0, 0], r[0, 1] = 1.0, 1.5                       # |k_1| >= 1: order 0
    r[1] = 1.0 + np.cos(0.7 * np.arange(17))          # DC + one sinusoid: E under the floor at order 3
    r[1, 0] += 1e-14
    r[2] = 0.9 ** np.arange(17)                       # an AR(1) process: runs to order 16
    r[3, 0], r[3, 1] = 1.0, -1.0                      # k_1 = -1: order 0
    r[4] = 0.0                                        # silent
    got = ops.whisper_lpc(_dev(r))
    a, sigma, order = W.lpc(r)
    assert order.tolist() == [0, 3, 16, 0, 0]
    assert np.array_equal(_np(got['order']), order)
    assert (_np(got['a'])[0, 1:] == 0).all() and (_np(got['a'])[1, 4:] == 0).all()
    assert np.array_equal(_np(got['a']) == 0, a == 0)
    print('whisper lpc crafted: a distance {:.2e}, sigma distance {:.2e}'.format(
        _rel(_np(got['a']), a), _rel(_np(got['sigma']), sigma)))
    assert _np(got['sigma'])[4] == 0.0 and (_np(got['sigma'])[:4] > 0).all()
    assert _np(got['a'])[4].tolist() == [1.0] + [0.0] * 16


# ---- batches --------------------------------------------------------------------------------------

def test_batch_equals_single_rows_and_repeats_and_device_tilt(wfx):
    from segan_pytorch_amd import ops
    T = 1500
    x = torch.stack([wfx['cases'][n]['x'][:T] for n in ('odd', 'partial', 'lag60', 'full', 'gap')])
    x = x.cuda().contiguous()
    lengths = [1500, 1000, 1024, 0, 77]
    seeds = [5, 2 ** 63 - 1, 0, 77, 123456789012345]
    tilts = [0.0, 0.9, 0.5, 0.25, 0.75]
    prev = _dev(np.asarray([0.1, 0.0, -0.2, 0.3, 0.0], dtype=np.float32))
    y, info = ops.whisper_rows(x, seeds, tilts, lengths, prev)
    y2, info2 = ops.whisper_rows(x, seeds, tilts, lengths, prev)
    assert _same(_np(y), _np(y2))
    for k in info:
        assert _same(_np(info[k]), _np(info2[k])), k
    for r in range(5):
        # alone, and in a row no longer than its own length: T beyond len takes no part
        for Tr in {T, max(lengths[r], 1)}:
            y1, i1 = ops.whisper_rows(x[r:r + 1, :Tr].contiguous(), seeds[r:r + 1], tilts[r:r + 1],
                                      [lengths[r]], prev[r:r + 1].contiguous())
            assert _same(_np(y1[0]), _np(y[r, :Tr])), (r, Tr)
            assert (_np(y[r, Tr:]) == 0).all()
            for k in info:
                assert _same(_np(i1[k]), _np(info[k][r:r + 1])), (r, Tr, k)
    assert _np(info['status']).tolist() == [0] * 5
    # device tensors for every per-row argument; a tilt outside [0, 1) flags its row only
    td = _dev(np.asarray([0.0, 1.0, 0.5, -0.25, float('nan')]))
    yd, infod = ops.whisper_rows(x, _dev(np.asarray(seeds, dtype=np.int64)), td,
                                 _dev(np.asarray(lengths, dtype=np.int32)), prev)
    assert _np(infod['status']).tolist() == [0, ops.WHISPER_TILT, 0, ops.WHISPER_TILT,
                                             ops.WHISPER_TILT]
    for r in (1, 3, 4):
        assert _same(_np(yd[r]), _np(x[r])) and _same(_np(infod['prev'][r]), _np(prev[r]))
    for r in (0, 2):
        assert _same(_np(yd[r]), _np(y[r])) and _same(_np(infod['prev'][r]), _np(info['prev'][r]))


def test_arguments_are_refused_before_any_launch():
    from segan_pytorch_amd import ops
    x = torch.zeros(2, 300, device='cuda')
    with pytest.raises(ValueError, match='tilts must lie in'):
        ops.whisper_rows(x, [1, 2], [0.0, 1.0])
    with pytest.raises(ValueError, match='tilts must lie in'):
        ops.whisper_rows(x, [1, 2], [float('nan'), 0.5])
    with pytest.raises(ValueError, match='seeds must lie in'):
        ops.whisper_rows(x, [-1, 2], [0.0, 0.5])
    with pytest.raises(ValueError, match='seeds must hold'):
        ops.whisper_rows(x, [1], [0.0, 0.5])
    with pytest.raises(ValueError, match='lag_hz'):
        ops.whisper_rows(x, [1, 2], [0.0, 0.5], lag_hz=-1.0)
    with pytest.raises(TypeError, match='out_dtype'):
        ops.whisper_rows(x, [1, 2], [0.0, 0.5], out_dtype=torch.float16)
    with pytest.raises(ValueError, match='j0'):
        ops.whisper_noise([1], -(1 << 20) - 1, 4)
    with pytest.raises(TypeError):
        ops.whisper_lpc(torch.zeros(3, 16, device='cuda', dtype=torch.float64))


def test_augment_whisper_call_and_apply(wfx):
    from segan_pytorch_amd import augment as A
    x = wfx['cases']['odd']['x'].numpy()
    out = A.Whisper(seed=1)(x)
    assert isinstance(out, torch.FloatTensor) and out.shape == (len(x),)
    assert torch.equal(out, A.Whisper(seed=1)(torch.from_numpy(x)))
    assert not torch.equal(out, torch.from_numpy(x))
    wh = A.Whisper(tilts=(0.25, 0.75), lag_hz=60.0, seed=3)
    xb = torch.stack([torch.from_numpy(x), torch.from_numpy(x)]).cuda()
    y, info = wh.apply(xb, seeds=[4, 4], tilt_ids=[1, 1])
    assert info['tilts'].tolist() == [0.75, 0.75] and torch.equal(y[0], y[1])
    o = W.whisper(x, 4, 0.75, lag_hz=60.0)
    assert _ulps32(_np(y[0]), o['out']) <= 1.0


# ---- the loader -----------------------------------------------------------------------------------

T_SLICE = 6000


@pytest.fixture(scope='module')
def shard(tmp_path_factory):
    from segan_pytorch_amd.datasets import PCMShardDataset, build_pcm_shard
    d = tmp_path_factory.mktemp('whisper_shard')
    cd, nd = d / 'clean', d / 'noisy'
    cd.mkdir()
    nd.mkdir()
    rng = np.random.default_rng(29)
    for i, n in enumerate((15100, 12100)):
        c = np.rint(GA.speech_like(n, 16000, 70 + i).astype(np.float64) * 40000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000,
                      (c + rng.standard_normal(n) * 300).astype(np.int16))
    assert build_pcm_shard(str(cd), str(nd), str(d / 'sh'), slice_size=T_SLICE, stride=0.5) == 7
    return PCMShardDataset(str(d / 'sh'))


def _loader(shard, **kw):
    from torch.utils.data import SequentialSampler
    from segan_pytorch_amd.datasets import PCMShardLoader
    return PCMShardLoader(shard, 4, 0.95, 'cuda', sampler=SequentialSampler(shard), num_workers=0,
                          **kw)


def _batches(loader):
    return [(list(n), c.cpu(), y.cpu(), i) for n, c, y, i in loader]


@pytest.mark.parametrize('stages', ['whisper', 'all'])
def test_loader_rows_recomposed_from_the_recorded_draws(shard, stages):
    """Whisper alone, and whisper, reverb, clip and noise together.  Per item, from the recorded
    draws and through the public ops on that item alone, in the loader's order; a batched row equals
    its own call bit for bit for every op involved, so the loader's noisy row must equal the
    recomposed one exactly."""
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    wh = A.Whisper()
    kw = dict(whisper=wh, whisper_prob=0.7, whisper_seed=[1, 3], record_whisper=True)
    noises = rbank = None
    if stages == 'all':
        noises = A.NoiseBank(GA.noise_bank())
        rbank = A.RIRBank([GR.rir_bank()[i] for i in (6, 11, 7)])
        kw.update(reverb=A.Reverb(rbank), reverb_prob=0.6, reverb_seed=2, record_reverb=True,
                  distort=A.Distort([A.Clip()]), distort_prob=0.6, distort_seed=12,
                  record_distort=True, additive=A.Additive(noises), additive_prob=0.5,
                  additive_seed=3, record_additive=True)
    ld = _loader(shard, **kw)
    got = _batches(ld)
    plain = _batches(_loader(shard))
    assert len(got) == len(plain) == 2
    seen = set()
    for k, ((names, clean, noisy, _), (pn, pc, py, _)) in enumerate(zip(got, plain)):
        assert torch.equal(clean, pc)
        recs = [getattr(ld, s + '_records') for s in ('whisper', 'reverb', 'distort', 'additive')]
        rw, rr, rd, ra = (None if rec is None else rec[k] for rec in recs)
        wsel, rsel, dsel, asel = ([] if rec is None else rec['index'].tolist()
                                  for rec in (rw, rr, rd, ra))
        B = len(names)
        pcm = np.stack([np.array(shard.data[4 * k + r]) for r in range(B)])
        first = shard._first[4 * k:4 * k + B]
        first_d = _dev(first)
        dry = ((2.0 / 65535.0) * (pcm[:, 0].astype(np.float64) - 32767.0) + 1.0).astype(np.float32)
        for r in range(B):
            wave, prev = _dev(dry[r, 1:]), _scalar(0.0 if first[r] else dry[r, 0])
            want = pn[r]
            if r in wsel:
                j = wsel.index(r)
                assert torch.equal(rw['wave'][j], wave) and torch.equal(rw['wave_prev'][j], prev)
                out, wi = ops.whisper_rows(wave[None].contiguous(), rw['seeds'][j:j + 1],
                                           rw['tilts'][j:j + 1], None, prev[None].contiguous(),
                                           lag_hz=wh.lag_hz)
                wave, prev = out[0], wi['prev'][0]
                assert torch.equal(rw['out'][j], wave) and int(wi['status'][0]) == 0
                assert rw['tilts'][j] == wh.tilts[rw['tilt_ids'][j]]
                want += '_whisper'
            if r in rsel:
                j = rsel.index(r)
                assert torch.equal(rr['wave'][j], wave) and torch.equal(rr['wave_prev'][j], prev)
                wet, ri = ops.reverb_rows(wave[None].contiguous(), rbank, rr['rir_ids'][j:j + 1],
                                          None, prev[None].contiguous())
                wave, prev = wet[0], ri['prev'][0]
                assert torch.equal(rr['wet'][j], wave)
                want += '_reverb'
            if r in dsel:
                j = dsel.index(r)
                assert torch.equal(rd['wave'][j], wave) and torch.equal(rd['wave_prev'][j], prev)
                jj = rd['clip']['index'].tolist().index(j)
                out, ci = ops.clip_rows(wave[None].contiguous(), rd['clip']['factors'][jj:jj + 1],
                                        None, prev[None].contiguous())
                wave, prev = out[0], ci['prev'][0]
                assert torch.equal(rd['out'][j], wave)
                want += '_clip'
            if r in asel:
                if r not in wsel and r not in rsel and r not in dsel:
                    prev = _scalar(dry[r, 0])      # additive alone takes the stored sample as it is
                j = asel.index(r)
                assert torch.equal(ra['wave'][j], wave) and torch.equal(ra['wave_prev'][j], prev)
                level = ops.asl_p56(wave[None].contiguous())
                mixed, mi = ops.additive_mix(wave[None].contiguous(), noises.data('cuda'),
                                             ra['abs_starts'][j:j + 1], ra['snrs'][j:j + 1],
                                             level['asl_ms'], None, prev[None].contiguous())
                wave, prev = mixed[0], mi['prev'][0]
                assert torch.equal(ra['mixed'][j], wave)
                want += '_additive'
            assert names[r] == want
            if r in wsel or r in rsel or r in dsel or r in asel:
                row = torch.empty(1, T_SLICE, device='cuda')
                ops.preemph_rows(wave[None].contiguous(), prev[None].contiguous(),
                                 first_d[r:r + 1].contiguous(), row, 0.95)
                assert torch.equal(noisy[r], row[0].cpu()), (k, r)
                assert not torch.equal(noisy[r], py[r])
            else:
                assert torch.equal(noisy[r], py[r])
            seen.add((r in wsel, r in rsel, r in dsel, r in asel))
    if stages == 'all':      # an item that all four stages took, and whisper followed by each other one
        assert (True, True, True, True) in seen, seen
        assert any(s[0] and s[3] for s in seen) and any(s[0] and s[1] for s in seen), seen
    else:
        assert seen == {(True, False, False, False), (False, False, False, False)}, seen


def test_loader_without_whisper_is_unchanged(shard):
    from segan_pytorch_amd import augment as A
    noises = A.NoiseBank(GA.noise_bank())
    kw = dict(additive_prob=0.5, additive_seed=7)
    a = _batches(_loader(shard, additive=A.Additive(noises, seed=1), **kw))
    b = _batches(_loader(shard, additive=A.Additive(noises, seed=1), whisper=None, whisper_prob=0.3,
                         whisper_seed=5, **kw))
    c = _batches(_loader(shard, additive=A.Additive(noises, seed=1), whisper=A.Whisper(),
                         whisper_prob=0.0, whisper_seed=5, **kw))
    for other in (b, c):
        assert len(a) == len(other) == 2
        for u, v in zip(a, other):
            assert u[0] == v[0] and all(torch.equal(p, q) for p, q in zip(u[1:], v[1:]))


# ---- scripts/whisper_wavs.py ----------------------------------------------------------------------

def test_whisper_wavs_writes_a_repeatable_copy(tmp_path, wfx):
    import json
    import whisper_wavs
    src = tmp_path / 'in'
    src.mkdir()
    for name in ('odd', 'partial'):
        wavfile.write(str(src / (name + '.wav')), 16000,
                      np.rint(wfx['cases'][name]['x'].numpy() * 32768).astype(np.int16))
    for out in ('a', 'b'):
        whisper_wavs.main([str(src), str(tmp_path / out), '--seed', '4', '--tilts', '0.5'])
    log = json.load(open(str(tmp_path / 'a' / 'whisper.json')))
    assert sorted(log['files']) == ['odd.wav', 'partial.wav'] and log['lag_hz'] == 120.0
    for name in log['files']:
        ra, a = wavfile.read(str(tmp_path / 'a' / name))
        _, b = wavfile.read(str(tmp_path / 'b' / name))
        _, x = wavfile.read(str(src / name))
        assert ra == 16000 and a.dtype == np.int16 and a.shape == x.shape
        assert np.array_equal(a, b) and not np.array_equal(a, x)
        rec = log['files'][name]
        assert rec['status'] == 0 and rec['tilt'] == 0.5 and rec['minorder'] == 16
        o = W.whisper(x.astype(np.float32) / np.float32(32768), rec['seed'], 0.5)
        want = np.clip(np.rint(o['out'].astype(np.float32).astype(np.float64) * 32768), -32768, 32767)
        assert np.abs(a - want).max() <= 1
