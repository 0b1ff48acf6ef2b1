"""Clipping, chunk removal and band limiting without a GPU: the float64
oracle (scripts/distort_oracle.py) against literal loops and np.convolve, `lowpass_bank`, the
fixture tests/golden/distort.pt (recipe scripts/make_golden_distort.py), the draws of Clip / Chop /
BandLimit / Distort, the loader's selection / naming / hand-over logic with the device ops replaced
by host stand-ins, the train.py flags and the C ABI."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import distort_oracle as D  # noqa: E402
import make_golden_distort as G  # noqa: E402


@pytest.fixture(scope='module')
def dfx():
    return load_golden('distort.pt')


# ---- the oracle ---------------------------------------------------------------------------------

def literal_fir(x, h, n, prev):
    """y[m] = h[0] xe[m] + sum_k h[k] (xe[m-k] + xe[m+k]), m = -1 .. n-1, as two loops."""
    def at(i):
        if i == -1:
            return 0.0 if prev is None else float(prev)
        return float(x[i]) if 0 <= i < n else 0.0
    out = []
    for m in range(-1, n):
        acc = float(h[0]) * at(m)
        for k in range(1, len(h)):
            acc = acc + float(h[k]) * (at(m - k) + at(m + k))
        out.append(acc)
    return np.array(out[1:] + [0.0] * (len(x) - n)), out[0]


@pytest.mark.parametrize('K', [0, 1, 3, 12])
@pytest.mark.parametrize('prev', [None, 0.7])
def test_fir_oracle_equals_the_double_loop(K, prev):
    rng = np.random.default_rng(7 + K)
    x = rng.standard_normal(9).astype(np.float32)
    h = rng.standard_normal(K + 1)
    for n in (9, 4, 1, 0):
        y, p = D.fir(x, h, n, prev)
        yl, pl = literal_fir(x, h, n, prev)
        assert np.array_equal(y, yl) and p == pl, (K, n)      # the same order: bit for bit
        assert not y[n:].any()
    y, p = D.fir(x, [1.0], None, prev)
    assert np.array_equal(y, x.astype(np.float64)) and p == (0.0 if prev is None else prev)


def test_fir_oracle_agrees_with_convolve():
    rng = np.random.default_rng(3)
    for K, h in G.filters():
        for T, n, prev in ((700, None, 0.4), (77, 50, None)):
            x = rng.uniform(-1, 1, T).astype(np.float32)
            y, p = D.fir(x, h, n, prev)
            yc, pc = D.fir_convolve(x, h, n, prev)
            bound = 2 * (K + 1) * 2.0 ** -53 * np.abs(h).sum() * max(np.abs(x).max(), abs(prev or 0))
            assert D.fir_bound(h, max(np.abs(x).max(), abs(prev or 0))) == bound
            assert max(np.abs(y - yc).max(), abs(p - pc)) <= bound, K


def test_clip_and_chop_oracle_on_tiny_inputs():
    x = np.array([0.1, -0.8, 0.4, 0.05, -0.2], dtype=np.float32)
    o = D.clip(x, 0.5, None, 0.9)
    thr = np.float32(0.5 * np.float64(np.float32(0.8)))
    assert o['m'] == np.float32(0.8) and o['thr'] == thr and o['nclipped'] == 1
    assert np.array_equal(o['y'], np.array([0.1, -thr, 0.4, 0.05, -0.2], dtype=np.float32))
    assert o['prev'] == thr and o['status'] == 0
    o = D.clip(x, 0.5, 1, -0.01)       # the peak of the row's own length only
    t1 = np.float32(0.5 * np.float64(np.float32(0.1)))
    assert o['m'] == np.float32(0.1) and o['thr'] == t1 and o['prev'] == np.float32(-0.01)
    assert o['y'][0] == t1 and np.array_equal(o['y'][1:], x[1:]) and o['nclipped'] == 1
    assert D.clip(x, 1.5)['status'] == D.CLIP_FACTOR and D.clip(x * 0, 0.5)['status'] == D.CLIP_SILENT
    q = np.array([0, 1, 1, 0, 1, 1, 1, 0, 1, 0], dtype=np.float64)
    xs = np.arange(1, 11, dtype=np.float32)
    o = D.chop(xs, q, 0.5, [0.0, 0.5, 0.99], [2, 0, 3])       # n = 6: k = 0, -, 5
    assert o['nactive'] == 6 and o['starts'].tolist() == [1, -1, 8] and o['nzeroed'] == 4
    assert o['y'].tolist() == [1, 0, 0, 4, 5, 6, 7, 8, 0, 0]
    o = D.chop(xs, q, 0.5, [0.5, 0.6], [4, 4], 7)             # n = 5: k = 2, 3; len = 7
    assert o['starts'].tolist() == [4, 5] and o['nzeroed'] == 3
    assert o['y'].tolist() == [1, 2, 3, 4, 0, 0, 0, 8, 9, 10]
    for c0 in (None, np.nan, 2.0):
        o = D.chop(xs, q, c0, [0.5], [4])
        assert o['status'] == D.CHOP_NOLEVEL and np.array_equal(o['y'], xs) and o['starts'][0] == -1


# ---- lowpass_bank -------------------------------------------------------------------------------

def test_lowpass_bank():
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import lowpass_bank
    cutoffs = (1000, 2000, 4000, 125)
    bank, K = lowpass_bank(cutoffs)
    assert K.dtype == np.int32 and K.tolist() == [256, 128, 64, 2048] and bank.shape == (4, 2049)
    assert bank.dtype == np.float64 and ops.FIR_MAX_K == 2048
    w = 2 * np.pi * np.arange(0, 8000.5, 0.5) / 16000.0
    for f, fc in enumerate(cutoffs):
        h = bank[f, :K[f] + 1]
        assert not bank[f, K[f] + 1:].any()
        assert abs(h[0] + 2 * h[1:].sum() - 1.0) <= 1e-15            # DC gain
        Ko, ho = D.lowpass(fc)
        assert Ko == K[f] and np.array_equal(ho, h)                  # the oracle's restatement
        H = h[0] + 2 * np.cos(np.outer(w, np.arange(1, K[f] + 1))) @ h[1:]
        f6 = 0.5 * np.nonzero(H < 0.5)[0][0]                         # first crossing of -6 dB
        assert abs(f6 - fc) <= 0.02 * fc, (fc, f6)
    assert lowpass_bank((500,), zeros=8)[1].tolist() == [128]
    with pytest.raises(ValueError, match='K = 2049 > 2048'):
        lowpass_bank((1000, 124.95))
    for bad in ((), (0,), (8000,), (-5,)):
        with pytest.raises(ValueError, match='cutoffs'):
            lowpass_bank(bad)


# ---- the fixture --------------------------------------------------------------------------------

def test_fixture_cases_and_margins(dfx):
    assert dfx['clip_cases'] == G.CLIP_CASES and dfx['chop_cases'] == G.CHOP_CASES
    assert dfx['fir_cases'] == G.FIR_CASES and dfx['fir_batch'] == G.FIR_BATCH
    assert dfx['filters'] == list(G.FILTERS) and dfx['margin'] == G.MARGIN == 1e-9
    cc = G.CLIP_CASES
    assert {rc['T'] for rc in cc.values()} == {1, 77, 2048 + 3, 16384}
    assert any(rc['factor'] == 1.0 for rc in cc.values())
    assert any(rc.get('scale') == 0.0 for rc in cc.values())
    assert {rc.get('length') for rc in cc.values()} >= {None, 0, 1500}
    for name, rc in cc.items():
        x = G.signal(rc)
        assert G.sha(x) == dfx['sha']['clip_' + name]
        o, want = D.clip(x, rc['factor'], rc.get('length'), rc['prev']), dfx['clip'][name]
        assert (float(o['m']), float(o['thr']), float(o['prev']), o['nclipped'], o['status']) == (
            want['m'], want['thr'], want['prev'], want['nclipped'], want['status']), name
        assert G.sha(o['y']) == want['y_sha']
    assert any(abs(rc['prev']) > dfx['clip'][k]['thr'] > 0 for k, rc in cc.items())
    for name, rc in G.CHOP_CASES.items():
        x, q, c0, margin, o = G.chop_case(rc)
        want = dfx['chop'][name]
        assert G.sha(x) == dfx['sha']['chop_' + name]
        assert margin > G.MARGIN and margin == want['margin'], (name, margin)
        assert (c0 is None) == np.isnan(want['c0']) and (c0 is None or c0 == want['c0'])
        assert (o['starts'].tolist(), o['nactive'], o['nzeroed'], o['status']) == (
            want['starts'], want['nactive'], want['nzeroed'], want['status']), name
        assert G.sha(o['y']) == want['y_sha']
        assert int(np.count_nonzero(o['y'] != x)) <= o['nzeroed']
    h = dfx['chop']
    assert h['spread']['starts'][0] < 1024 < h['spread']['starts'][1]
    assert h['spread']['starts'][2] + 4000 > 16384 and h['overlap']['starts'][1] == -1
    assert h['partial']['nzeroed'] == 4100 - h['partial']['starts'][0] > 0
    assert {len(rc['u']) for rc in G.CHOP_CASES.values()} >= {1, 8} and 5000 % 1024
    assert dfx['K'] == [K for K, _ in G.filters()] == [0, 1, 256, 64, 2048]
    assert [G.sha(hh) for _, hh in G.filters()] == dfx['filter_sha']
    fc = G.FIR_CASES
    assert fc['k_over_T']['T'] == 77 and fc['kmax_tile']['T'] == G.FIR_TILE + 1
    assert len(G.FIR_BATCH['filt']) == 5 and max(G.FIR_BATCH['filt']) == len(G.FILTERS)
    fl = G.filters()
    for name, rc in fc.items():
        x = G.signal(rc)
        assert G.sha(x) == dfx['sha']['fir_' + name]
        K, hh = fl[rc['filt']]
        y, p = D.fir(x, hh, rc.get('length'), G.fir_prev(rc))
        assert np.array_equal(y, dfx['fir'][name]['y'].numpy()) and p == dfx['fir'][name]['prev']
        assert dfx['fir'][name]['convolve_dev'] <= dfx['fir'][name]['bound']


# ---- draws --------------------------------------------------------------------------------------

def test_draw_order_and_repeatability():
    from segan_pytorch_amd import augment as A
    clip, chop, band = A.Clip(), A.Chop(), A.BandLimit()
    assert clip.factors.tolist() == [0.1, 0.2, 0.3, 0.4, 0.5]
    assert (chop.max_chops, chop.durs, chop.srate) == (3, (0.05, 0.3), 16000)
    assert band.cutoffs.tolist() == [1000, 2000, 4000] and band.K.tolist() == [256, 128, 64]
    # Clip: one vectorised draw of indices
    r = np.random.default_rng(5)
    want = clip.factors[np.random.default_rng(5).integers(5, size=40)]
    assert np.array_equal(clip.draw(r, 40), want) and set(want) == set(clip.factors)
    assert np.array_equal(clip.draw(r, 2, [0.25, 1.0]), [0.25, 1.0])
    for bad in ([0.0, 0.5], [0.5], [1.5, 0.5]):
        with pytest.raises(ValueError, match=r'\(0, 1\]'):
            clip.draw(r, 2, bad)
    # Chop: counts, then durations, then positions
    g = np.random.default_rng(6)
    count = g.integers(1, 4, size=50)
    dur = np.rint(g.uniform(0.05, 0.3, size=(50, 3)) * 16000)
    u = g.random((50, 3))
    gu, gd = chop.draw(np.random.default_rng(6), 50)
    assert np.array_equal(gu, u) and gd.dtype == np.int32 and gu.shape == gd.shape == (50, 3)
    for r_ in range(50):
        assert gd[r_, :count[r_]].tolist() == dur[r_, :count[r_]].tolist()
        assert not gd[r_, count[r_]:].any() and gd[r_, 0] >= 800
    assert set(count) == {1, 2, 3} and gd.max() <= 4800 and (gu >= 0).all() and (gu < 1).all()
    # BandLimit: one vectorised draw of ids
    assert np.array_equal(band.draw(np.random.default_rng(7), 30),
                          np.random.default_rng(7).integers(3, size=30))
    with pytest.raises(ValueError, match='filter ids'):
        band.draw(np.random.default_rng(7), 2, [0, 3])
    # the objects' own generators are seeded
    assert np.array_equal(A.Clip(seed=3).draw(A.Clip(seed=3).rng, 9), A.Clip(seed=3).draw(
        np.random.default_rng(3), 9))
    # Distort: kinds of all rows first, numbered in the order clip, chop, bandlimit
    d = A.Distort([band, clip, chop], seed=11)
    assert d.enabled == ['clip', 'chop', 'bandlimit']
    assert np.array_equal(d.draw_kinds(np.random.default_rng(11), 20),
                          np.random.default_rng(11).integers(3, size=20))
    assert A.Distort({'chop': chop}).enabled == ['chop']
    for bad in ([], [clip, A.Clip()], {'clop': clip}, [object()]):
        with pytest.raises(ValueError, match='Distort'):
            A.Distort(bad)
    with pytest.raises(ValueError, match='Chop: durs'):
        A.Chop(durs=(0.3, 0.05))
    with pytest.raises(ValueError, match='max_chops'):
        A.Chop(max_chops=9)
    with pytest.raises(ValueError, match=r'\(0, 1\]'):
        A.Clip(factors=(0.5, 1.1))


class _Spy(object):
    """Stands in for one kind inside Distort: takes the real object's draws from the generator it
    is given and records them with the rows it received."""

    def __init__(self, kind, log, real):
        self.kind, self.log, self.real = kind, log, real

    def apply(self, wave, generator=None, prev=None, lengths=None):
        drawn = self.real.draw(generator, wave.shape[0])
        self.log.append((self.kind, wave.clone(), prev.clone(), drawn, lengths))
        mark = {'clip': 1.0, 'chop': 2.0, 'bandlimit': 3.0}[self.kind]
        return wave + mark, dict(prev=prev - mark,
                                 status=torch.full((wave.shape[0],), int(mark), dtype=torch.int32))


def test_distort_draws_in_the_documented_order_and_scatters(monkeypatch):
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    monkeypatch.setattr(ops, '_chk', lambda t, name, ndim=None: t)
    real = dict(clip=A.Clip(), chop=A.Chop(), bandlimit=A.BandLimit())
    log = []
    d = A.Distort({k: _Spy(k, log, v) for k, v in real.items()})
    rows, T = 12, 6
    wave = torch.arange(rows * T, dtype=torch.float32).view(rows, T)
    prev = torch.arange(rows, dtype=torch.float32) * 10
    lens = np.arange(rows) % T + 1
    out, info = d.apply(wave, generator=np.random.default_rng(21), prev=prev, lengths=lens)
    g = np.random.default_rng(21)
    code = g.integers(3, size=rows)
    assert set(code) == {0, 1, 2}
    assert info['kinds'].tolist() == [A.DISTORT_KINDS[c] for c in code]
    assert [e[0] for e in log] == ['clip', 'chop', 'bandlimit']
    for c, (kind, w, p, drawn, ln) in enumerate(log):
        idx = np.nonzero(code == c)[0]
        want = real[kind].draw(g, len(idx))          # the same generator, in this order
        if kind == 'chop':
            assert np.array_equal(drawn[0], want[0]) and np.array_equal(drawn[1], want[1])
        else:
            assert np.array_equal(drawn, want)
        assert torch.equal(w, wave[idx]) and torch.equal(p, prev[idx]) and ln.tolist() == lens[idx].tolist()
        assert info[kind]['index'].tolist() == idx.tolist()
        assert torch.equal(out[idx], wave[idx] + (c + 1)) and torch.equal(info['prev'][idx], prev[idx] - (c + 1))
        assert info['status'][idx].tolist() == [c + 1] * len(idx)
    # repeatable from the seed; one kind alone takes the whole batch in one call
    log.clear()
    out2, info2 = d.apply(wave, generator=np.random.default_rng(21), prev=prev, lengths=lens)
    assert torch.equal(out, out2) and info2['kinds'].tolist() == info['kinds'].tolist()
    log.clear()
    solo = A.Distort([_Spy('chop', log, real['chop'])])
    out3, info3 = solo.apply(wave, generator=np.random.default_rng(2))
    assert len(log) == 1 and torch.equal(log[0][1], wave) and not log[0][2].any()
    assert torch.equal(out3, wave + 2) and set(info3['kinds']) == {'chop'}


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    x = torch.zeros(2, 8)
    for obj in (A.Clip(seed=1), A.Chop(seed=1), A.BandLimit(seed=1), A.Distort([A.Clip()], seed=1)):
        with pytest.raises(RuntimeError, match='MI355X'):
            obj.apply(x)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match='MI355X'):
                obj(np.zeros(10))
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.clip_rows(x, [0.5, 0.5])
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.chop_rows(x, x.double(), torch.zeros(2).double(), [[0.5], [0.5]], [[1], [1]])
    with pytest.raises(RuntimeError, match='MI355X'):
        ops.fir_rows(x, torch.ones(1, 1).double(), torch.zeros(1, dtype=torch.int32), [0, 0])
    with pytest.raises(RuntimeError, match='MI355X'):
        A.BandLimit().data('cpu')


# ---- the loader's logic, the device ops replaced by host stand-ins -------------------------------

T_SLICE = 64


class HostReverb(object):
    """Stands in for augment.Reverb: doubles the wave, draws ids from the generator it is given."""

    def __init__(self):
        self.calls = []

    def apply(self, clean, generator=None, rir_ids=None, lengths=None, prev=None):
        ids = generator.integers(5, size=clean.shape[0])
        self.calls.append(dict(wave=clean.clone(), prev=prev.clone(), ids=ids))
        return clean * 2, dict(prev=prev * 2 + 1, status=torch.zeros(len(ids), dtype=torch.int32),
                               rir_ids=ids, taps=ids + 1, delays=ids)


class HostDistort(object):
    """Stands in for augment.Distort: negates the wave, draws the kinds from its generator."""

    def __init__(self):
        self.calls = []

    def apply(self, wave, generator=None, prev=None, lengths=None):
        code = generator.integers(3, size=wave.shape[0])
        self.calls.append(dict(wave=wave.clone(), prev=prev.clone(), code=code))
        kinds = np.asarray(['clip', 'chop', 'bandlimit'], dtype=object)[code]
        return -wave, dict(kinds=kinds, prev=-prev - 3,
                           status=torch.zeros(len(code), dtype=torch.int32))


def host_ops(monkeypatch):
    from segan_pytorch_amd import ops

    def norm(v):
        return ((2.0 / 65535.0) * (v.double() - 32767.0) + 1.0).float()

    def pcm16_prep(pcm, first, coef):
        c, n = norm(pcm[:, 0]), norm(pcm[:, 1])
        return c[:, 1:].clone(), n[:, 1:].clone()

    def pcm16_wave(pcm, index=None):
        w = norm(pcm[torch.as_tensor(index), 0])
        return w[:, 1:].clone(), w[:, 0].clone()

    def preemph_rows(x, prev, first, out, coef, index=None):
        out[torch.as_tensor(index)] = x + 100 * prev[:, None]      # recognisable, not a filter
        return out

    monkeypatch.setattr(ops, 'pcm16_prep', pcm16_prep)
    monkeypatch.setattr(ops, 'pcm16_wave', pcm16_wave)
    monkeypatch.setattr(ops, 'preemph_rows', preemph_rows)


def host_additive(seed=1):
    from segan_pytorch_amd.augment import Additive, NoiseBank

    class HostAdditive(Additive):
        def mix(self, clean, generator=None, prev=None, **kw):
            ids, sn, st = self.bank.draw(generator, np.full(len(clean), clean.shape[1]),
                                         self.snr_levels)
            self.seen.append(dict(wave=clean.clone(), prev=prev.clone()))
            return clean + 7, dict(prev=prev + 7, noise_ids=ids, snrs=sn, starts=st)

    rng = np.random.default_rng(4)
    a = HostAdditive(NoiseBank([rng.standard_normal(500).astype(np.float32) for _ in range(3)]),
                     seed=seed)
    a.seen = []
    return a


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


N_BATCH = 4


def run_loader(shard, **kw):
    from segan_pytorch_amd.datasets import PCMShardLoader
    ld = PCMShardLoader(shard, 4, 0.95, 'cpu', num_workers=0, record_additive=True,
                        record_reverb=True, record_distort=True, **kw)
    out = [ld._prep(shard.gather(range(4 * k, 4 * k + 4))) for k in range(N_BATCH)]
    return out, ld


def test_loader_three_stages(shard, monkeypatch):
    host_ops(monkeypatch)
    plain, _ = run_loader(shard)
    kw = dict(additive_prob=0.5, additive_seed=3, reverb_prob=0.5, reverb_seed=8)
    two, ld2 = run_loader(shard, additive=host_additive(), reverb=HostReverb(), **kw)
    rv, ds = HostReverb(), HostDistort()
    three, ld3 = run_loader(shard, additive=host_additive(), reverb=rv, distort=ds, distort_prob=0.6,
                            distort_seed=13, **kw)
    seen = set()
    for k in range(N_BATCH):
        names, clean, noisy, _ = three[k]
        pn, pc, py, _ = plain[k]
        assert torch.equal(clean, pc)      # clean is never touched
        ra2, rr2 = ld2.additive_records[k], ld2.reverb_records[k]
        ra, rr, rd = ld3.additive_records[k], ld3.reverb_records[k], ld3.distort_records[k]
        # the reverb and additive selections and draws do not move when distortion is on
        for a, b, keys in ((ra2, ra, ('index', 'noise_ids', 'snrs', 'starts')),
                           (rr2, rr, ('index', 'rir_ids'))):
            assert (a is None) == (b is None)
            for key in keys if a is not None else ():
                assert np.array_equal(a[key], b[key]), key
        asel = [] if ra is None else ra['index'].tolist()
        rsel = [] if rr is None else rr['index'].tolist()
        dsel = [] if rd is None else rd['index'].tolist()
        pcm = torch.from_numpy(np.stack([np.array(shard.data[4 * k + i]) for i in range(4)]))
        w = ((2.0 / 65535.0) * (pcm[:, 0].double() - 32767.0) + 1.0).float()
        first = shard._first[4 * k:4 * k + 4]
        for i in range(4):
            wave, prev = w[i, 1:], (torch.tensor(0.0) if first[i] else w[i, 0])
            want = pn[i]
            if i in rsel:
                wave, prev, want = wave * 2, (torch.tensor(0.0) if first[i] else w[i, 0]) * 2 + 1, \
                    want + '_reverb'
            elif i not in dsel:
                prev = w[i, 0]              # additive alone takes the stored sample as it is
            if i in dsel:
                j = dsel.index(i)
                assert torch.equal(rd['wave'][j], wave) and rd['wave_prev'][j] == prev
                wave, prev, want = -wave, -prev - 3, want + '_' + rd['kinds'][j]
                assert rd['kinds'][j] in ('clip', 'chop', 'bandlimit')
            if i in asel:                    # noise is mixed into the wave the stages before left
                j = asel.index(i)
                assert torch.equal(ra['wave'][j], wave) and ra['wave_prev'][j] == prev
                wave, prev, want = wave + 7, prev + 7, want + '_additive'
            assert names[i] == want
            if i in rsel or i in dsel or i in asel:
                assert torch.equal(noisy[i], wave + 100 * prev), (k, i)
            else:
                assert torch.equal(noisy[i], py[i])
            seen.add((i in rsel, i in dsel, i in asel))
    assert seen >= {(True, True, True), (True, True, False), (False, True, True),
                    (False, True, False), (True, False, True)}, seen
    # its own seeded stream: the same seed repeats, another seed does not
    d1, d2, d3 = HostDistort(), HostDistort(), HostDistort()
    one, ld1 = run_loader(shard, distort=d1, distort_seed=13)
    run_loader(shard, distort=d2, distort_seed=13)
    _, ldo = run_loader(shard, distort=d3, distort_seed=14)
    assert all(n.rsplit('_', 1)[1] in ('clip', 'chop', 'bandlimit') for b in one for n in b[0])
    assert all(np.array_equal(a['code'], b['code']) for a, b in zip(d1.calls, d2.calls))
    assert any(not np.array_equal(a['code'], b['code']) for a, b in zip(d1.calls, d3.calls))
    assert ld1.additive_records == [] and ld1.reverb_records == []


def test_loader_without_distort_is_unchanged(shard, monkeypatch):
    host_ops(monkeypatch)
    kw = dict(additive_prob=0.5, additive_seed=3, reverb_prob=0.5, reverb_seed=8)
    base, ldb = run_loader(shard, additive=host_additive(), reverb=HostReverb(), **kw)
    none, ldn = run_loader(shard, additive=host_additive(), reverb=HostReverb(), distort=None,
                           distort_prob=0.3, distort_seed=4, **kw)
    zero, ldz = run_loader(shard, additive=host_additive(), reverb=HostReverb(),
                           distort=HostDistort(), distort_prob=0.0, distort_seed=4, **kw)
    assert ldn.distort_records == [] and ldz.distort_records == [None] * N_BATCH
    for other, ld in ((none, ldn), (zero, ldz)):
        for a, b in zip(base, other):
            assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
        for ra, rb in zip(ldb.additive_records, ld.additive_records):
            assert (ra is None) == (rb is None)
            if ra is not None:
                assert all(np.array_equal(ra[key], rb[key])
                           for key in ('index', 'noise_ids', 'snrs', 'starts'))
    plain, _ = run_loader(shard)
    off, _ = run_loader(shard, distort=None)
    for a, b in zip(plain, off):
        assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))


def test_loader_checks_the_probability():
    from segan_pytorch_amd.datasets import PCMShardLoader
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError, match='distort_prob'):
            PCMShardLoader(None, 2, 0.95, 'cpu', distort=object(), distort_prob=p)


# ---- train.py flags -----------------------------------------------------------------------------

def test_train_flags_parse_and_go_with_pcm_shard():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.distort is None and d.distort_prob == 1.0 and d.clip_factors == [0.1, 0.2, 0.3, 0.4, 0.5]
    assert d.chop_max == 3 and d.chop_durs == [0.05, 0.3]
    assert d.bandlimit_cutoffs == [1000, 2000, 4000] and train.check_distort_flags(d) is False
    o = p.parse_args(['--pcm_shard', 'sh', '--distort', 'clip', 'chop', 'bandlimit', '--distort_prob',
                      '0.7', '--clip_factors', '0.25', '1', '--chop_max', '8', '--chop_durs', '0.01',
                      '0.02', '--bandlimit_cutoffs', '125', '7999'])
    assert o.distort == ['clip', 'chop', 'bandlimit'] and o.distort_prob == 0.7
    assert o.clip_factors == [0.25, 1.0] and o.chop_max == 8 and o.chop_durs == [0.01, 0.02]
    assert train.check_distort_flags(o) is True
    assert train.check_reverb_flags(o) is False and train.check_additive_flags(o) is False
    o = p.parse_args(['--pcm_shard', 'sh', '--distort', 'chop', '--reverb_rirs', 'd',
                      '--additive_noises', 'n'])
    assert train.check_distort_flags(o) and train.check_reverb_flags(o)
    with pytest.raises(SystemExit):      # argparse: not one of the kinds
        p.parse_args(['--pcm_shard', 'sh', '--distort', 'echo'])
    sh = ['--pcm_shard', 'sh']
    for bad, msg in ((['--distort', 'clip'], 'only together with --pcm_shard'),
                     (['--distort', 'clip', '--synthetic', '8'], 'only together with'),
                     (sh + ['--distort_prob', '0.5'], 'needs --distort KIND'),
                     (sh + ['--clip_factors', '0.5'], 'needs --distort clip'),
                     (sh + ['--distort', 'chop', '--clip_factors', '0.5'], 'needs --distort clip'),
                     (sh + ['--distort', 'clip', '--chop_max', '2'], 'need --distort chop'),
                     (sh + ['--distort', 'clip', '--chop_durs', '0.1', '0.2'], 'need --distort chop'),
                     (sh + ['--distort', 'clip', '--bandlimit_cutoffs', '3000'],
                      'needs --distort bandlimit'),
                     (sh + ['--distort', 'clip', 'clip'], 'names a kind twice'),
                     (sh + ['--distort', 'clip', '--distort_prob', '1.5'], 'must lie in 0 .. 1'),
                     (sh + ['--distort', 'clip', '--distort_prob', '-0.5'], 'must lie in 0 .. 1'),
                     (sh + ['--distort', 'clip', '--clip_factors', '0.5', '0'], r'\(0, 1\]'),
                     (sh + ['--distort', 'clip', '--clip_factors', '1.01'], r'\(0, 1\]'),
                     (sh + ['--distort', 'chop', '--chop_max', '9'], 'must lie in 1 .. 8'),
                     (sh + ['--distort', 'chop', '--chop_max', '0'], 'must lie in 1 .. 8'),
                     (sh + ['--distort', 'chop', '--chop_durs', '0.3', '0.1'], 'LO <= HI'),
                     (sh + ['--distort', 'chop', '--chop_durs', '0', '0.1'], 'LO <= HI'),
                     (sh + ['--distort', 'bandlimit', '--bandlimit_cutoffs', '8000'],
                      'below 8000 Hz'),
                     (sh + ['--distort', 'bandlimit', '--bandlimit_cutoffs', '0'], 'below 8000 Hz'),
                     (sh + ['--distort', 'bandlimit', '--bandlimit_cutoffs', '2000', '124'],
                      'K = 2065 taps a side')):
        with pytest.raises(SystemExit, match=msg):
            train.check_distort_flags(p.parse_args(bad))
        with pytest.raises(SystemExit, match=msg):      # before anything touches a device
            train.main(p.parse_args(bad))
    for flag in ('--distort', '--distort_prob', '--clip_factors', '--chop_max', '--chop_durs',
                 '--bandlimit_cutoffs'):
        assert flag in train.__doc__, flag
    # the defaults of the flags are the defaults of the classes
    from segan_pytorch_amd import augment as A
    assert A.Clip().factors.tolist() == list(train.CLIP_FACTORS)
    assert (A.Chop().max_chops, A.Chop().durs) == (train.CHOP_MAX, train.CHOP_DURS)
    assert A.BandLimit().cutoffs.tolist() == list(train.BANDLIMIT_CUTOFFS)
    assert train.DISTORT_KINDS == A.DISTORT_KINDS


# ---- C ABI --------------------------------------------------------------------------------------

DISTORT_SYMBOLS = ('segan_clip_rows', 'segan_chop_rows', 'segan_fir_rows')


def test_header_lib_and_abi_agree():
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17
    for name, val in (('SEGAN_CHOP_MAX', ops.CHOP_MAX), ('SEGAN_FIR_MAX_K', ops.FIR_MAX_K),
                      ('SEGAN_FIR_TILE', ops.FIR_TILE), ('SEGAN_CLIP_ST_SILENT', ops.CLIP_SILENT),
                      ('SEGAN_CLIP_ST_FACTOR', ops.CLIP_FACTOR),
                      ('SEGAN_CHOP_ST_NOLEVEL', ops.CHOP_NOLEVEL), ('SEGAN_FIR_ST_ID', ops.FIR_ID)):
        assert H.macro(name) == val, name
    assert (ops.CHOP_MAX, ops.FIR_MAX_K, ops.FIR_TILE) == (D.CHOP_MAX, D.FIR_MAX_K, G.FIR_TILE)
    assert (ops.CLIP_SILENT, ops.CLIP_FACTOR, ops.CHOP_NOLEVEL) == (
        D.CLIP_SILENT, D.CLIP_FACTOR, D.CHOP_NOLEVEL)
    assert _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in DISTORT_SYMBOLS:
        assert len(H.args(name)) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and name in doc
    assert 'without a change of SEGAN_ABI_VERSION' in H.RAW[H.RAW.index('segan_clip_rows:'):]
    # arguments validated before any launch
    buf = torch.zeros(64)
    q = buf.data_ptr()
    assert lib.segan_clip_rows(None, None, None, q, 1, 16, q, None, q, q, q, q, None) == -1
    assert b'clip_rows' in lib.segan_last_error()
    assert lib.segan_clip_rows(q, None, q, q, 1, 16, q, None, q, q, q, q, None) == -1
    assert b'go together' in lib.segan_last_error()
    assert lib.segan_clip_rows(q, None, None, q, 65536, 16, q, None, q, q, q, q, None) == -1
    assert lib.segan_chop_rows(q, None, q, q, q, q, 1, 16, 9, q, q, q, q, q, None) == -1
    assert b'chunks per row' in lib.segan_last_error()
    assert lib.segan_chop_rows(q, None, q, q, q, q, 1, 16, 0, q, q, q, q, q, None) == -1
    assert lib.segan_chop_rows(q, None, q, q, q, q, 0, 16, 1, q, q, q, q, q, None) == -1
    assert lib.segan_fir_rows(q, None, None, q, q, 1, 2049, q, 1, 16, q, 0, q, q, None) == -1
    assert b'kmax' in lib.segan_last_error()
    assert lib.segan_fir_rows(q, None, None, q, q, 0, 4, q, 1, 16, q, 0, q, q, None) == -1
    assert lib.segan_fir_rows(q, None, None, q, q, 1, 4, q, 1, 16, q, 1, q, q, None) == -1
    assert b'y_dtype' in lib.segan_last_error()
    assert lib.segan_fir_rows(q, None, None, q, q, 1, 4, q, 1, 16, q, 0, None, q, None) == -1
