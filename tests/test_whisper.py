"""Whispered speech without a GPU: the numpy oracle scripts/whisper_oracle.py
against what a whisper has to be (no pitch, the voiced row's energy contour), its excitation and
guards, the fixture's recipe, and the host logic: augment.Whisper's draws, the loader's stage
order, names and random streams, train.py's flags, the C ABI.

The caps of the oracle properties are conditions on the definition, set before the oracle was
written; the rows are periodic (f0 = 110, 180, 240 Hz, T = 16384, peak 0.5 so that the peak guard
stays off), made here.  The energy rows use tilt 0: a tilt is meant to move energy (at tau = 0.5
the excitation carries 6 dB less around the first formant), which the tilt test checks."""
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_whisper as G  # noqa: E402
import whisper_oracle as W  # noqa: E402
from test_distort import HostDistort, HostReverb, host_additive, host_ops  # noqa: E402

F0S = (110, 180, 240)


@pytest.fixture(scope='module')
def rows():
    """(x, oracle result at tilt 0) per f0, computed once"""
    out = {}
    for f0 in F0S:
        x = W.voiced(f0, 16384, f0)
        out[f0] = (x, W.whisper(x, 12345 + f0, 0.0))
    return out


def pitch_peak(x, f0):
    """the largest normalised autocorrelation within +-3 lags of the pitch period, samples 4096..8192"""
    s = np.asarray(x, dtype=np.float64)[4096:8192]
    p = int(round(W.SRATE / f0))
    return max(np.dot(s[:-l], s[l:]) / np.sqrt(np.dot(s[:-l], s[:-l]) * np.dot(s[l:], s[l:]))
               for l in range(p - 3, p + 4))


# ---- oracle properties ----------------------------------------------------------------------------

@pytest.mark.parametrize('f0', F0S)
def test_whisper_has_no_pitch_and_keeps_the_energy_contour(f0, rows):
    x, o = rows[f0]
    y = o['out']
    assert o['status'] == 0 and o['peak'] <= 1.0 and abs(np.abs(x).max() - 0.5) < 1e-4
    pin, pout = pitch_peak(x, f0), pitch_peak(y, f0)
    ex = (x.astype(np.float64) ** 2).reshape(-1, 1024).sum(1)
    ey = (y ** 2).reshape(-1, 1024).sum(1)
    sel = ex > 1e-3 * ex.max()
    seg = 10 * np.log10(ey[sel] / ex[sel])
    tot = 10 * np.log10(ey.sum() / ex.sum())
    print('f0 {}: pitch peak in {:.3f} out {:.3f}, segments {:+.2f} .. {:+.2f} dB, total {:+.2f} dB'
          .format(f0, pin, pout, seg.min(), seg.max(), tot))
    assert pin > 0.8
    assert pout < 0.2
    assert sel.sum() >= 8 and np.abs(seg).max() <= 3.0
    assert abs(tot) <= 0.5


def test_excitation():
    # (the three Random123 vectors are asserted when the oracle is imported; once more here)
    W._check_vectors()
    ones = 0xFFFFFFFF
    assert [int(v) for v in W.philox4x32_10((ones,) * 4, (ones,) * 2)] == [
        0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert W.C == float(np.sqrt(np.float64((2 ** 64 - 1) / 3)))
    u = W.noise(7, 0, 1 << 16)
    assert abs(u.mean()) <= 0.02 and abs(u.var() - 1.0) <= 0.02
    # one continuous sequence: any window of it is the same numbers; another seed, other numbers
    assert np.array_equal(W.noise(7, -513, 600)[513:], u[:87])
    assert not np.array_equal(W.noise(8, 0, 64), u[:64])
    assert np.array_equal(W.noise(7, 0, 64, np.longdouble).astype(np.float64), u[:64])


def test_tilt_moves_energy_upwards(rows):
    x, flat = rows[180]
    tilted = W.whisper(x, 12345 + 180, 0.9)

    def high_over_low(y):
        p = np.abs(np.fft.rfft(y)) ** 2
        f = np.fft.rfftfreq(len(y), 1.0 / W.SRATE)
        return p[f > 4000].sum() / p[f < 1000].sum()

    assert high_over_low(tilted['out']) > 4 * high_over_low(flat['out'])
    assert np.array_equal(tilted['a'], flat['a']) and np.array_equal(tilted['sigma'], flat['sigma'])


def test_peak_guard_and_status():
    x = W.voiced(180, 4096, 1, peak=0.9)
    o = W.whisper(x, 5, 0.0)
    assert o['peak'] > 1.0 and np.abs(o['y']).max() == 1.0      # exactly 1 before the fp32 rounding
    assert np.abs(o['out']).max() <= 1.0 and abs(o['prev_out']) <= 1.0
    for tilt in (-0.1, 1.0, float('nan')):
        b = W.whisper(x, 5, tilt, prev=0.25)
        assert b['status'] == W.WHISPER_TILT and np.array_equal(b['out'], x)
        assert b['prev_out'] == np.float32(0.25)
    z = W.whisper(np.zeros(700, np.float32), 5, 0.5)
    assert z['status'] == W.WHISPER_SILENT and z['nsilent'] == 700 // 256 + 2
    assert not z['out'].any()
    e = W.whisper(x[:77], 5, 0.5, length=0, prev=0.25)          # only the preceding sample
    assert e['status'] == 0 and e['prev_out'] != 0 and not e['out'].any()
    # zero beyond len, and T beyond len takes no part
    p = W.whisper(x, 5, 0.5, length=1000, prev=0.1)
    q = W.whisper(x[:1000], 5, 0.5, prev=0.1)
    assert not p['out'][1000:].any() and np.array_equal(p['out'][:1000], q['out'])


def test_levinson_guards():
    r = np.zeros((4, 17))
    r[0, 0], r[0, 1] = 1.0, 1.5
    r[1] = 1.0 + np.cos(0.7 * np.arange(17))
    r[1, 0] += 1e-14
    r[2] = 0.9 ** np.arange(17)
    a, sigma, order = W.lpc(r)
    assert order.tolist() == [0, 3, 16, 0]
    assert a[0].tolist() == [1.0] + [0.0] * 16 and sigma[0] == np.sqrt(1.0 / 192.0)
    assert not a[1, 4:].any() and a[1, 1:4].all()
    assert 0 < sigma[1] ** 2 * 192 <= 2.0 ** -40 * r[1, 0]
    assert abs(a[2, 1] + 0.9) < 1e-12 and np.abs(a[2, 2:]).max() < 1e-12
    assert a[3].tolist() == [1.0] + [0.0] * 16 and sigma[3] == 0


def test_tables():
    from segan_pytorch_amd import ops
    w, g = ops.whisper_tables(120.0)
    assert np.array_equal(w, W.hann()) and np.array_equal(g, W.lag_window(120.0))
    assert np.abs(w[:256] + w[256:] - 1.0).max() < 1e-15 and abs((w ** 2).sum() - 192.0) < 1e-12
    assert g[0] == 1.0 and (np.diff(g) < 0).all()
    assert (ops.WHISPER_N, ops.WHISPER_H, ops.WHISPER_P, ops.WHISPER_WU) == (W.N, W.H, W.P, W.WU)
    for bad in (-1.0, 1001.0, float('nan')):
        with pytest.raises(ValueError, match='lag_hz'):
            ops.whisper_tables(bad)


def test_fixture_is_what_the_recipe_makes():
    fx = load_golden('whisper.pt')
    assert set(fx['cases']) == set(G.CASES) and fx['max_move'] == 1e-10
    Ts = sorted({len(c['x']) for c in fx['cases'].values()})
    assert Ts == [1, 77, 255, 256, 257, 300, 1500, 4096]
    for name in ('short', 'gap', 'guard', 'lag60'):
        c = G.make_case(name, G.CASES[name])
        f = fx['cases'][name]
        assert torch.equal(c['x'], f['x']) and torch.equal(c['out'], f['out']), name
        assert torch.equal(c['r'], f['r']) and torch.equal(c['a'], f['a']), name
        assert (c['status'], c['nsilent'], c['minorder']) == (f['status'], f['nsilent'],
                                                              f['minorder'])
    worst = max(c['move']['y'] for c in fx['cases'].values())
    assert 0 < worst == fx['largest_move']['y'] <= 1e-10
    assert fx['cases']['guard']['peak'] > 1 and fx['cases']['gap']['nsilent'] > 2
    assert fx['cases']['lag60']['move']['y'] <= 1e-10
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'whisper.pt')) < 1 << 20


# ---- augment.Whisper ------------------------------------------------------------------------------

def test_draw_order_and_shapes():
    from segan_pytorch_amd import augment as A
    wh = A.Whisper(seed=9)
    assert wh.tilts.tolist() == [0.0, 0.5, 0.9] and wh.lag_hz == 120.0
    seeds, ids = wh.draw(np.random.default_rng(3), 5)
    ref = np.random.default_rng(3)
    want_seeds = ref.integers(0, 2 ** 63, size=5, dtype=np.int64)
    want_ids = ref.integers(3, size=5)
    assert seeds.dtype == np.int64 and seeds.shape == (5,) and np.array_equal(seeds, want_seeds)
    assert ids.dtype == np.int64 and ids.shape == (5,) and np.array_equal(ids, want_ids)
    assert (seeds >= 0).all()
    # values passed in are kept and not drawn
    rng = np.random.default_rng(3)
    s2, i2 = wh.draw(rng, 5, seeds=[1, 2, 3, 4, 5])
    assert s2.tolist() == [1, 2, 3, 4, 5] and np.array_equal(
        i2, np.random.default_rng(3).integers(3, size=5))
    for bad in (dict(seeds=[1, 2]), dict(seeds=[-1, 0, 0, 0, 0]), dict(tilt_ids=[0, 1, 2, 3, 0])):
        with pytest.raises(ValueError, match='Whisper'):
            wh.draw(np.random.default_rng(0), 5, **bad)
    for tilts in ((), (1.0,), (-0.1, 0.5), (float('nan'),)):
        with pytest.raises(ValueError, match='tilts'):
            A.Whisper(tilts=tilts)
    with pytest.raises(ValueError, match='lag_hz'):
        A.Whisper(lag_hz=-5)
    assert A.DISTORT_KINDS == ('clip', 'chop', 'bandlimit') and not hasattr(A.Whisper, 'kind')
    with pytest.raises((TypeError, RuntimeError, ValueError)):      # no CPU path
        wh.apply(torch.zeros(2, 300))


# ---- the loader -----------------------------------------------------------------------------------

T_SLICE = 64
N_BATCH = 4


class HostWhisper(object):
    """Stands in for augment.Whisper: the wave plus 0.5, draws like `Whisper.draw`."""

    def __init__(self):
        self.calls = []

    def apply(self, wave, generator=None, seeds=None, tilt_ids=None, lengths=None, prev=None):
        seeds = generator.integers(0, 2 ** 63, size=wave.shape[0], dtype=np.int64)
        ids = generator.integers(3, size=wave.shape[0])
        self.calls.append(dict(wave=wave.clone(), prev=prev.clone(), seeds=seeds, ids=ids))
        return wave + 0.5, dict(prev=prev * 3 - 2, seeds=seeds, tilt_ids=ids,
                                status=torch.zeros(len(ids), dtype=torch.int32))


@pytest.fixture()
def shard(tmp_path):
    from segan_pytorch_amd.datasets import PCMShardDataset, build_pcm_shard
    cd, nd = tmp_path / 'clean', tmp_path / 'noisy'
    cd.mkdir()
    nd.mkdir()
    rng = np.random.default_rng(5)
    for i in range(3):
        c = (rng.standard_normal(232) * 3000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000, c)
    assert build_pcm_shard(str(cd), str(nd), str(tmp_path / 'sh'), slice_size=T_SLICE,
                           stride=0.5) >= 16
    return PCMShardDataset(str(tmp_path / 'sh'))


def run_loader(shard, record=True, **kw):
    from segan_pytorch_amd.datasets import PCMShardLoader
    if record:
        kw.update(record_additive=True, record_reverb=True, record_distort=True, record_whisper=True)
    ld = PCMShardLoader(shard, 4, 0.95, 'cpu', num_workers=0, **kw)
    out = [ld._prep(shard.gather(range(4 * k, 4 * k + 4))) for k in range(N_BATCH)]
    return out, ld


def test_stage_table():
    from segan_pytorch_amd import datasets
    assert datasets._STAGES[0] == ('whisper', 'apply', True, 'out')
    assert [s[0] for s in datasets._STAGES] == ['whisper', 'reverb', 'distort', 'additive']


def test_loader_four_stages_in_order(shard, monkeypatch):
    """A spy stands in for each stage: the order is whisper, reverb, distort, additive, every stage
    receives the rows as the stage before left them, the names say so, clean is untouched."""
    host_ops(monkeypatch)
    plain, _ = run_loader(shard)
    kw = dict(additive_prob=0.5, additive_seed=3, reverb_prob=0.5, reverb_seed=8, distort_prob=0.6,
              distort_seed=13)
    three, ld3 = run_loader(shard, record=False, record_additive=True, record_reverb=True,
                            record_distort=True, additive=host_additive(), reverb=HostReverb(),
                            distort=HostDistort(), **kw)
    wh = HostWhisper()
    four, ld = run_loader(shard, additive=host_additive(), reverb=HostReverb(), distort=HostDistort(),
                          whisper=wh, whisper_prob=0.6, whisper_seed=[0, 3], **kw)
    seen = set()
    for k in range(N_BATCH):
        names, clean, noisy, _ = four[k]
        pn, pc, py, _ = plain[k]
        assert torch.equal(clean, pc)
        rw, rr, rd, ra = (getattr(ld, s + '_records')[k]
                          for s in ('whisper', 'reverb', 'distort', 'additive'))
        # the three older stages select and draw what they did without the whisper stage
        for a, b, keys in ((ld3.additive_records[k], ra, ('index', 'noise_ids', 'snrs', 'starts')),
                           (ld3.reverb_records[k], rr, ('index', 'rir_ids')),
                           (ld3.distort_records[k], rd, ('index', 'kinds'))):
            assert (a is None) == (b is None)
            for key in keys if a is not None else ():
                assert np.array_equal(a[key], b[key]), key
        wsel, rsel, dsel, asel = ([] if rec is None else rec['index'].tolist()
                                  for rec in (rw, rr, rd, ra))
        pcm = torch.from_numpy(np.stack([np.array(shard.data[4 * k + i]) for i in range(4)]))
        w = ((2.0 / 65535.0) * (pcm[:, 0].double() - 32767.0) + 1.0).float()
        first = shard._first[4 * k:4 * k + 4]
        for i in range(4):
            wave, prev = w[i, 1:], (torch.tensor(0.0) if first[i] else w[i, 0])
            want = pn[i]
            for sel, rec, step, suffix in (
                    (wsel, rw, lambda v, p: (v + 0.5, p * 3 - 2), '_whisper'),
                    (rsel, rr, lambda v, p: (v * 2, p * 2 + 1), '_reverb'),
                    (dsel, rd, lambda v, p: (-v, -p - 3), None),
                    (asel, ra, lambda v, p: (v + 7, p + 7), '_additive')):
                if i not in sel:
                    continue
                j = sel.index(i)
                if suffix == '_additive' and not (i in wsel or i in rsel or i in dsel):
                    prev = w[i, 0]              # additive alone takes the stored sample as it is
                assert torch.equal(rec['wave'][j], wave) and rec['wave_prev'][j] == prev, (k, i)
                wave, prev = step(wave, prev)
                want += suffix if suffix else '_' + rd['kinds'][j]
            assert names[i] == want
            if i in wsel or i in rsel or i in dsel or i in asel:
                assert torch.equal(noisy[i], wave + 100 * prev), (k, i)
            else:
                assert torch.equal(noisy[i], py[i])
            seen.add((i in wsel, i in rsel, i in dsel, i in asel))
    assert (True, True, True, True) in seen, seen
    assert any(s[0] and s[1] and not s[2] for s in seen), seen
    assert any(s[0] and not s[1] and s[2] for s in seen) and any(not s[0] for s in seen), seen
    full = [n for b in four for n in b[0] if n.count('_') >= 4 and '_whisper_reverb_' in n]
    assert full and all(re.search(r'_whisper_reverb_(clip|chop|bandlimit)_additive$', n)
                        for n in full), full
    # the stage's own seeded stream: selections first, then seeds, then tilt ids
    rng = np.random.default_rng([0, 3])
    for call, rec in zip(wh.calls, [r for r in ld.whisper_records if r is not None]):
        sel = np.nonzero(rng.random(4) < 0.6)[0]
        while len(sel) == 0:
            sel = np.nonzero(rng.random(4) < 0.6)[0]
        assert np.array_equal(rec['index'], sel)
        assert np.array_equal(call['seeds'], rng.integers(0, 2 ** 63, size=len(sel), dtype=np.int64))
        assert np.array_equal(call['ids'], rng.integers(3, size=len(sel)))


def test_loader_without_whisper_is_unchanged(shard, monkeypatch):
    from segan_pytorch_amd.datasets import PCMShardLoader
    host_ops(monkeypatch)
    kw = dict(additive_prob=0.5, additive_seed=3, reverb_prob=0.5, reverb_seed=8, distort_prob=0.6,
              distort_seed=13)

    def run(**extra):
        # built without the keyword at all when `extra` is empty
        ld = PCMShardLoader(shard, 4, 0.95, 'cpu', num_workers=0, record_additive=True,
                            record_reverb=True, record_distort=True, additive=host_additive(),
                            reverb=HostReverb(), distort=HostDistort(), **kw, **extra)
        return [ld._prep(shard.gather(range(4 * k, 4 * k + 4))) for k in range(N_BATCH)], ld

    base, ldb = run()
    none, ldn = run(whisper=None, whisper_prob=0.3, whisper_seed=4, record_whisper=True)
    zero, ldz = run(whisper=HostWhisper(), whisper_prob=0.0, whisper_seed=4, record_whisper=True)
    assert ldb.whisper is None and ldb.whisper_records is None
    assert ldn.whisper_records == [] and ldz.whisper_records == [None] * N_BATCH
    for other, ld in ((none, ldn), (zero, ldz)):
        for a, b in zip(base, other):
            assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
        for stage, keys in (('additive', ('index', 'noise_ids', 'snrs', 'starts')),
                            ('reverb', ('index', 'rir_ids')), ('distort', ('index', 'kinds'))):
            for ra, rb in zip(getattr(ldb, stage + '_records'), getattr(ld, stage + '_records')):
                assert (ra is None) == (rb is None)
                if ra is not None:
                    assert all(np.array_equal(ra[key], rb[key]) for key in keys)
    assert not any('whisper' in n for b in none + zero for n in b[0])
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError, match='whisper_prob'):
            PCMShardLoader(None, 2, 0.95, 'cpu', whisper=object(), whisper_prob=p)


# ---- train.py flags -------------------------------------------------------------------------------

def test_train_flags_parse_and_go_with_pcm_shard():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.whisper is False and d.whisper_prob == 1.0 and d.whisper_tilts == [0.0, 0.5, 0.9]
    assert d.whisper_lag_hz == 120.0 and train.check_whisper_flags(d) is False
    o = p.parse_args(['--pcm_shard', 'sh', '--whisper', '--whisper_prob', '0.5', '--whisper_tilts',
                      '0', '0.99', '--whisper_lag_hz', '60'])
    assert o.whisper and o.whisper_prob == 0.5 and o.whisper_tilts == [0.0, 0.99]
    assert o.whisper_lag_hz == 60.0 and train.check_whisper_flags(o) is True
    assert not train.check_distort_flags(o) and not train.check_reverb_flags(o)
    assert not train.check_additive_flags(o)
    o = p.parse_args(['--pcm_shard', 'sh', '--whisper', '--distort', 'clip', '--reverb_rirs', 'd',
                      '--additive_noises', 'n'])
    assert train.check_whisper_flags(o) and train.check_distort_flags(o)
    assert train.check_reverb_flags(o) and train.check_additive_flags(o)
    sh = ['--pcm_shard', 'sh']
    for bad, msg in ((['--whisper'], 'only together with --pcm_shard'),
                     (['--whisper', '--synthetic', '8'], 'only together with'),
                     (sh + ['--synthetic', '8', '--whisper'], 'whispers the batches'),
                     (sh + ['--whisper_prob', '0.5'], 'need --whisper'),
                     (sh + ['--whisper_tilts', '0.5'], 'need --whisper'),
                     (sh + ['--whisper_lag_hz', '60'], 'need --whisper'),
                     (sh + ['--whisper', '--whisper_prob', '1.5'], 'must lie in 0 .. 1'),
                     (sh + ['--whisper', '--whisper_prob', '-0.5'], 'must lie in 0 .. 1'),
                     (sh + ['--whisper', '--whisper_tilts', '0.5', '1'], r'\[0, 1\)'),
                     (sh + ['--whisper', '--whisper_tilts', '-0.1'], r'\[0, 1\)'),
                     (sh + ['--whisper', '--whisper_tilts', 'nan'], r'\[0, 1\)'),
                     (sh + ['--whisper', '--whisper_lag_hz', '-1'], '0 .. 1000 Hz'),
                     (sh + ['--whisper', '--whisper_lag_hz', '1001'], '0 .. 1000 Hz')):
        with pytest.raises(SystemExit, match=msg):
            train.check_whisper_flags(p.parse_args(bad))
        with pytest.raises(SystemExit, match=msg):      # before anything touches a device
            train.main(p.parse_args(bad))
    for flag in ('--whisper', '--whisper_prob', '--whisper_tilts', '--whisper_lag_hz'):
        assert flag in train.__doc__, flag
    from segan_pytorch_amd import augment as A
    assert A.Whisper().tilts.tolist() == list(train.WHISPER_TILTS)
    assert A.Whisper().lag_hz == train.WHISPER_LAG_HZ
    assert train.DISTORT_KINDS == A.DISTORT_KINDS == ('clip', 'chop', 'bandlimit')
    # the messages of the three older checks are what they were
    for check, bad, msg in (
            (train.check_additive_flags, sh + ['--additive_prob', '0.5'],
             '--additive_snrs / --additive_prob need --additive_noises DIR'),
            (train.check_additive_flags, ['--additive_noises', 'n'],
             '--additive_noises mixes noise into the batches of a pcm16 shard on the GPU'),
            (train.check_reverb_flags, sh + ['--reverb_resample'],
             '--reverb_resample needs --reverb_rirs DIR'),
            (train.check_reverb_flags, ['--reverb_rirs', 'd'], '--reverb_rirs reverberates the batches'),
            (train.check_distort_flags, sh + ['--distort', 'chop', '--clip_factors', '0.5'],
             '--clip_factors needs --distort clip'),
            (train.check_distort_flags, ['--distort', 'clip'], '--distort distorts the batches')):
        with pytest.raises(SystemExit, match=msg):
            check(p.parse_args(bad))


# ---- C ABI ----------------------------------------------------------------------------------------

WHISPER_SYMBOLS = ('segan_whisper_noise', 'segan_whisper_lags', 'segan_whisper_lpc',
                   'segan_whisper_synth', 'segan_whisper_rows')


def test_header_lib_and_abi_agree():
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17
    for name, val in (('SEGAN_WHISPER_N', ops.WHISPER_N), ('SEGAN_WHISPER_H', ops.WHISPER_H),
                      ('SEGAN_WHISPER_P', ops.WHISPER_P), ('SEGAN_WHISPER_WU', ops.WHISPER_WU),
                      ('SEGAN_WHISPER_ST_SILENT', ops.WHISPER_SILENT),
                      ('SEGAN_WHISPER_ST_TILT', ops.WHISPER_TILT)):
        assert H.macro(name) == val, name
    assert (ops.WHISPER_SILENT, ops.WHISPER_TILT) == (W.WHISPER_SILENT, W.WHISPER_TILT)
    assert _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in WHISPER_SYMBOLS + ('segan_whisper_frames', 'segan_whisper_ws_doubles'):
        assert len(H.args(name, '(?:int|long long)')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and name in doc
    assert 'without a change of SEGAN_ABI_VERSION' in H.RAW[H.RAW.index('segan_whisper_rows:'):]
    assert 'segan_whisper.hip' in open(os.path.join(ROOT, 'Makefile')).read()
    # host arithmetic of the library, and arguments validated before any launch
    assert [lib.segan_whisper_frames(T) for T in (1, 255, 256, 16384)] == [2, 2, 3, 66]
    assert lib.segan_whisper_ws_doubles(300, 16384) == 300 * 66 * (17 + 17 + 1 + 512) + 9900
    q = torch.zeros(64).data_ptr()
    assert lib.segan_whisper_noise(None, 0, 4, 1, q, None) == -1
    assert b'whisper_noise' in lib.segan_last_error()
    assert lib.segan_whisper_noise(q, -(1 << 20) - 1, 4, 1, q, None) == -1
    assert b'j0' in lib.segan_last_error()
    assert lib.segan_whisper_lags(q, None, None, q, q, 65536, 16, q, None) == -1
    assert lib.segan_whisper_lags(q, None, None, None, q, 1, 16, q, None) == -1
    assert lib.segan_whisper_lpc(q, 0, q, q, q, None) == -1
    assert b'whisper_lpc' in lib.segan_last_error()
    assert lib.segan_whisper_synth(q, None, None, q, q, q, q, q, q, q, 1, 16, q, 10, q, 0, q, q, q,
                                   q, q, None) == -1
    assert b'workspace' in lib.segan_last_error()
    assert lib.segan_whisper_synth(q, None, None, q, q, q, q, q, q, q, 1, 16, q, 1024, q, 1, q, q,
                                   q, q, q, None) == -1
    assert b'y_dtype' in lib.segan_last_error()
    assert lib.segan_whisper_rows(q, None, None, q, q, q, q, 1, 16, q, 10, q, 0, q, q, q, q, q,
                                  None) == -1
    assert b'workspace' in lib.segan_last_error()
