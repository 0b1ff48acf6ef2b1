"""Clipping, chunk removal and band limiting on the MI355X (ops.clip_rows, ops.chop_rows,
ops.fir_rows, augment.Clip / Chop / BandLimit / Distort, PCMShardLoader's distort stage, train.py
--distort) against the float64 oracle scripts/distort_oracle.py on the cases of
tests/golden/distort.pt (recipe scripts/make_golden_distort.py).

Bounds.  The clip and the chop are exact: every output is compared bit for bit (the chop with the
envelope q and the threshold c0 copied from the device, so that the comparison does not depend on
the level kernel's last bits; end to end on fixture rows only, whose q clears c0 by 1e-9 of its
peak where the device's q and c0 are within 1e-12 and 1e-13).  The FIR's fp64 output is compared
bit for bit with the oracle that sums in the kernel's order, and within 2 (K + 1) 2^-53 sum|h|
max|x| with np.convolve, which sums in another; the fp32 output within one fp32 ulp of the rounded
fp64 oracle (measured: equal)."""
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
import distort_oracle as D  # noqa: E402
import make_golden_additive as GA  # noqa: E402
import make_golden_distort as G  # noqa: E402
import make_golden_reverb as GR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dfx():
    return load_golden('distort.pt')


@pytest.fixture(scope='module')
def fbank():
    bank, K = G.filter_bank()
    return _dev(bank), _dev(K), G.filters()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scalar(v):
    return torch.tensor(float(np.float32(v)), dtype=torch.float32, device='cuda')


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    """Bit equality of two float arrays (NaN-free here; -0.0 and 0.0 differ)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- clip ---------------------------------------------------------------------------------------

def _check_clip(y, info, r, x, factor, length, prev):
    o = D.clip(x, factor, length, prev)
    got = (float(info['m'][r]), float(info['thr'][r]), int(info['nclipped'][r]),
           int(info['status'][r]))
    assert got == (float(o['m']), float(o['thr']), o['nclipped'], o['status']), (got, o)
    assert _same(_np(y[r]), o['y'])
    if prev is not None:
        assert _np(info['prev'][r]).tobytes() == np.float32(o['prev']).tobytes()
    return o


@pytest.mark.parametrize('name', list(G.CLIP_CASES))
def test_clip_cases_bit_equal(name, dfx):
    from segan_pytorch_amd import ops
    rc = G.CLIP_CASES[name]
    x = G.signal(rc)
    lengths = None if 'length' not in rc else [rc['length']]
    y, info = ops.clip_rows(_dev(x[None]), [rc['factor']], lengths,
                            _dev(np.array([rc['prev']], dtype=np.float32)))
    o = _check_clip(y, info, 0, x, rc['factor'], rc.get('length'), np.float32(rc['prev']))
    want = dfx['clip'][name]
    assert (float(o['m']), float(o['thr']), o['nclipped'], o['status'], G.sha(_np(y[0]))) == (
        want['m'], want['thr'], want['nclipped'], want['status'], want['y_sha'])
    y2, info2 = ops.clip_rows(_dev(x[None]), [rc['factor']], lengths)      # without prev
    assert torch.equal(y, y2) and 'prev' not in info2


def test_clip_batch_equals_single_rows_and_device_factors():
    from segan_pytorch_amd import ops
    T = 2051
    names = ('odd', 'factor1', 'partial')
    xs = np.stack([G.signal(G.CLIP_CASES[n]) for n in names] + [np.zeros(T, np.float32)] * 2)
    xs[4] = G.signal(dict(T=T, seed=29)) * np.float32(1.7)
    f = [G.CLIP_CASES[n]['factor'] for n in names] + [0.3, 0.25]
    lens = [T, T, 1500, 700, 0]
    prev = np.array([0.001, 0.7, -0.25, 0.2, -0.9], dtype=np.float32)
    y, info = ops.clip_rows(_dev(xs), f, lens, _dev(prev))
    for r in range(5):
        _check_clip(y, info, r, xs[r], f[r], lens[r], prev[r])
        y1, i1 = ops.clip_rows(_dev(xs[r:r + 1]), f[r:r + 1], lens[r:r + 1], _dev(prev[r:r + 1]))
        assert torch.equal(y1[0], y[r])
        for key in ('m', 'thr', 'nclipped', 'status', 'prev'):
            assert torch.equal(i1[key][0], info[key][r]), key
    assert info['status'].tolist() == [0, 0, 0, ops.CLIP_SILENT, ops.CLIP_SILENT]
    # device factors and lengths are taken as they are; the kernel flags a factor it cannot use
    fd = _dev(np.array([0.1, 0.0, 1.5, float('nan'), 0.25]))
    yd, idv = ops.clip_rows(_dev(xs), fd, _dev(np.array(lens, dtype=np.int32)), _dev(prev))
    assert idv['status'].tolist() == [0, ops.CLIP_FACTOR, ops.CLIP_FACTOR,
                                      ops.CLIP_FACTOR | ops.CLIP_SILENT, ops.CLIP_SILENT]
    assert torch.equal(yd[0], y[0]) and torch.equal(yd[1:], _dev(xs)[1:])
    assert torch.equal(idv['prev'][1:], _dev(prev)[1:]) and idv['nclipped'][1:].tolist() == [0] * 4


# ---- chop ---------------------------------------------------------------------------------------

def _check_chop(y, info, r, x, q, c0, u, dur, length):
    o = D.chop(x, q, None if np.isnan(c0) else c0, u, dur, length)
    got = (_np(info['starts'][r]).tolist(), int(info['nactive'][r]), int(info['nzeroed'][r]),
           int(info['status'][r]))
    assert got == (o['starts'].tolist(), o['nactive'], o['nzeroed'], o['status']), (got, o)
    assert _same(_np(y[r]), o['y'])
    return o


@pytest.mark.parametrize('name', list(G.CHOP_CASES))
def test_chop_cases_with_the_device_level(name, dfx):
    """The kernel alone (q and c0 copied from the device: integer-exact whatever the level
    kernel's last bits), then end to end through augment.Chop against the fixture, whose numbers
    come from the oracle's own q and c0."""
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import Chop
    rc = G.CHOP_CASES[name]
    x = G.signal(rc)
    lengths = None if 'length' not in rc else [rc['length']]
    xd = _dev(x[None])
    level = ops.asl_p56_stages(xd, 16000, 16, lengths)
    y, info = ops.chop_rows(xd, level['q'], level['c0'], [rc['u']], [rc['dur']], lengths)
    _check_chop(y, info, 0, x, _np(level['q'][0]), float(level['c0'][0]), rc['u'], rc['dur'],
                rc.get('length'))
    ye, ie = Chop(max_chops=len(rc['u'])).apply(xd, u=np.array([rc['u']]), dur=np.array([rc['dur']]),
                                                lengths=lengths)
    want = dfx['chop'][name]
    assert (_np(ie['starts'][0]).tolist(), int(ie['nactive'][0]), int(ie['nzeroed'][0]),
            int(ie['status'][0]), G.sha(_np(ye[0]))) == (
        want['starts'], want['nactive'], want['nzeroed'], want['status'], want['y_sha'])
    assert torch.equal(ye, y)


def test_chop_synthetic_levels_slabs_and_batch():
    """q and c0 made by hand: targets at chosen ranks in the first slab, across a slab boundary and
    at the last active sample; c0 NaN; nothing active; C = 1 and 8; T no multiple of the slab; len <
    T; and a batched row against its own call."""
    from segan_pytorch_amd import ops
    T = 3 * 1024 + 77
    rng = np.random.default_rng(8)
    x = rng.uniform(-1, 1, (6, T)).astype(np.float32)
    q = rng.uniform(0, 1, (6, T))
    q[1] = 0.0
    q[1, [3, 1023, 1024, 2047, 2048, T - 1]] = 1.0       # six active samples around the slab edges
    q[2, :1100] = 0.0                                    # the first slab holds nothing
    c0 = np.array([0.5, 0.5, 0.25, float('nan'), 2.0, 0.9])
    lens = [T, T, T - 5, T, T, 1500]
    u8 = np.array([[0.0, 0.999999, 0.5, 0.25, 0.75, 0.1, 0.9, 0.6],
                   [0.0, 0.17, 0.34, 0.5, 0.67, 0.84, 0.99, 0.5],
                   [0.0, 0.3, 0.3001, 0.99, 0.5, 0.5, 0.0, 0.7],
                   [0.1] * 8, [0.2] * 8,
                   [0.999, 0.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])
    d8 = np.array([[5, 50, 700, 0, 1200, 1, 0, 64],
                   [1, 1, 1, 1, 1, 1, 1, 2000],
                   [10, 600, 600, 4000, 0, 0, 3, 1],
                   [9] * 8, [9] * 8,
                   [4000, 1, 0, 30, 0, 0, 0, 2]], dtype=np.int32)
    xd, qd, cd = _dev(x), _dev(q), _dev(c0)
    for C in (8, 1):
        u, d = u8[:, :C], d8[:, :C]
        y, info = ops.chop_rows(xd, qd, cd, u, d, lens)
        for r in range(6):
            o = _check_chop(y, info, r, x[r], q[r], c0[r], u[r], d[r], lens[r])
            y1, i1 = ops.chop_rows(xd[r:r + 1], qd[r:r + 1], cd[r:r + 1], u[r:r + 1], d[r:r + 1],
                                   lens[r:r + 1])
            assert torch.equal(y1[0], y[r])
            for key in ('starts', 'nactive', 'nzeroed', 'status'):
                assert torch.equal(i1[key][0], info[key][r]), key
        assert info['status'].tolist() == [0, 0, 0, ops.CHOP_NOLEVEL, ops.CHOP_NOLEVEL, 0]
        assert torch.equal(y[3:5], xd[3:5]) and (info['starts'][3:5] == -1).all()
    y, info = ops.chop_rows(xd, qd, cd, u8, d8, lens)
    assert _np(info['starts'][1]).tolist() == [3, 1023, 1024, 2047, 2048, T - 1, T - 1, 2047]
    s2 = info['starts'][2]
    assert int(info['nactive'][1]) == 6 and int(s2[s2 >= 0].min()) >= 1100 and int((s2 >= 0).sum()) == 6
    # device u / dur give the same
    yd, idv = ops.chop_rows(xd, qd, cd, _dev(u8), _dev(d8), _dev(np.array(lens, dtype=np.int32)))
    assert torch.equal(yd, y) and torch.equal(idv['starts'], info['starts'])


# ---- fir ----------------------------------------------------------------------------------------

def _check_fir(y64, p64, y32, p32, x, h, length, prev):
    yo, po = D.fir(x, h, length, prev)
    assert _same(y64, yo) and float(p64) == po                           # the kernel's order
    yc, pc = D.fir_convolve(x, h, length, prev)
    bound = D.fir_bound(h, max(float(np.abs(x).max()), abs(float(prev or 0.0))))
    assert max(np.abs(y64 - yc).max(), abs(float(p64) - pc)) <= bound
    want = np.concatenate(([po], yo)).astype(np.float32)
    got = np.concatenate(([p32], y32))
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want)).astype(np.float64)
    assert got.dtype == np.float32 and ulps.max() <= 1.0
    n = len(x) if length is None else length
    assert not y64[n:].any() and not y32[n:].any()
    return float(ulps.max())


@pytest.mark.parametrize('name', list(G.FIR_CASES))
def test_fir_cases(name, dfx, fbank):
    from segan_pytorch_amd import ops
    bank, K, fl = fbank
    rc = G.FIR_CASES[name]
    x = G.signal(rc)
    lengths = None if 'length' not in rc else [rc['length']]
    prev = None if 'prev' not in rc else _dev(np.array([rc['prev']], dtype=np.float32))
    pv = G.fir_prev(rc)
    y64, i64 = ops.fir_rows(_dev(x[None]), bank, K, [rc['filt']], lengths, prev, torch.float64)
    y32, i32 = ops.fir_rows(_dev(x[None]), bank, K, [rc['filt']], lengths, prev)
    assert y64.dtype == i64['prev'].dtype == torch.float64 and y32.dtype == torch.float32
    assert i64['status'].tolist() == [0] and i32['status'].tolist() == [0]
    worst = _check_fir(_np(y64[0]), _np(i64['prev'][0]), _np(y32[0]), _np(i32['prev'][0]), x,
                       fl[rc['filt']][1], rc.get('length'), pv)
    print('fir', name, 'fp32 ulps', worst)
    assert _same(_np(y64[0]), dfx['fir'][name]['y'].numpy())
    assert float(i64['prev'][0]) == dfx['fir'][name]['prev']
    if name == 'identity':
        assert torch.equal(y32[0], _dev(x)) and float(i32['prev'][0]) == rc['prev']


def test_fir_batch_filters_per_row_and_an_id_outside_the_bank(fbank):
    from segan_pytorch_amd import ops
    bank, K, fl = fbank
    rc = G.FIR_BATCH
    x = np.stack([G.signal(dict(T=rc['T'], seed=s)) for s in rc['seeds']])
    prev = np.array(rc['prev'], dtype=np.float32)
    xd, pd = _dev(x), _dev(prev)
    y64, i64 = ops.fir_rows(xd, bank, K, rc['filt'], rc['lengths'], pd, torch.float64)
    y32, i32 = ops.fir_rows(xd, bank, K, rc['filt'], rc['lengths'], pd)
    bad = [f >= len(fl) for f in rc['filt']]
    assert i64['status'].tolist() == i32['status'].tolist() == [ops.FIR_ID if b else 0 for b in bad]
    for r, f in enumerate(rc['filt']):
        if bad[r]:      # copied unchanged, whatever its length
            assert torch.equal(y32[r], xd[r]) and torch.equal(y64[r], xd[r].double())
            assert float(i32['prev'][r]) == float(prev[r]) == float(i64['prev'][r])
        else:
            _check_fir(_np(y64[r]), _np(i64['prev'][r]), _np(y32[r]), _np(i32['prev'][r]), x[r],
                       fl[f][1], rc['lengths'][r], prev[r])
        for dt, yb, ib in ((torch.float64, y64, i64), (torch.float32, y32, i32)):
            y1, i1 = ops.fir_rows(xd[r:r + 1], bank, K, rc['filt'][r:r + 1], rc['lengths'][r:r + 1],
                                  pd[r:r + 1], dt)
            assert torch.equal(y1[0], yb[r]) and torch.equal(i1['prev'][0], ib['prev'][r])
    # device ids and lengths give the same
    yd, idv = ops.fir_rows(xd, bank, K, _dev(np.array(rc['filt'], dtype=np.int32)),
                           _dev(np.array(rc['lengths'], dtype=np.int32)), pd)
    assert torch.equal(yd, y32) and torch.equal(idv['prev'], i32['prev'])


# ---- arguments ----------------------------------------------------------------------------------

def test_arguments_are_refused_before_any_launch(fbank):
    from segan_pytorch_amd import ops
    bank, K, _ = fbank
    x = torch.zeros(2, 16, device='cuda')
    q, c0 = torch.zeros(2, 16, device='cuda', dtype=torch.float64), torch.zeros(
        2, device='cuda', dtype=torch.float64)
    big = torch.zeros(65536, 1, device='cuda')
    ok_u, ok_d = [[0.5], [0.5]], [[1], [1]]
    V, Ty = ValueError, TypeError
    for exc, msg, call in (
            (V, r'\(0, 1\]', lambda: ops.clip_rows(x, [0.5, 0.0])),
            (V, r'\(0, 1\]', lambda: ops.clip_rows(x, [0.5, 1.01])),
            (V, r'\(0, 1\]', lambda: ops.clip_rows(x, [0.5, float('nan')])),
            (V, 'factors must hold', lambda: ops.clip_rows(x, [0.5])),
            (V, 'device factors', lambda: ops.clip_rows(x, torch.ones(2, device='cuda'))),
            (V, '65535 rows', lambda: ops.clip_rows(big, [0.5] * 65536)),
            (V, 'lengths must lie', lambda: ops.clip_rows(x, [0.5, 0.5], [3, 17])),
            (V, 'device lengths', lambda: ops.clip_rows(x, [0.5, 0.5], torch.ones(2, device='cuda'))),
            (V, 'prev must hold', lambda: ops.clip_rows(x, [0.5, 0.5], None, x[0, :3].contiguous())),
            (Ty, 'float32', lambda: ops.clip_rows(x.double(), [0.5, 0.5])),
            (V, '2 dims', lambda: ops.clip_rows(x[0], [0.5])),
            (V, 'empty', lambda: ops.clip_rows(x[:, :0], [0.5, 0.5])),
            (Ty, 'q must be', lambda: ops.chop_rows(x, q.float(), c0, ok_u, ok_d)),
            (Ty, 'q must be', lambda: ops.chop_rows(x, q[:, :8].contiguous(), c0, ok_u, ok_d)),
            (Ty, 'c0 must be', lambda: ops.chop_rows(x, q, c0[:1], ok_u, ok_d)),
            (Ty, 'c0 must be', lambda: ops.chop_rows(x, q, [0.1, 0.1], ok_u, ok_d)),
            (V, 'C from 1 to 8', lambda: ops.chop_rows(x, q, c0, [[0.5] * 9] * 2, [[1] * 9] * 2)),
            (V, 'C from 1 to 8', lambda: ops.chop_rows(x, q, c0, [0.5, 0.5], [1, 1])),
            (V, r'u must lie in \[0, 1\)', lambda: ops.chop_rows(x, q, c0, [[1.0], [0.5]], ok_d)),
            (V, r'u must lie in \[0, 1\)', lambda: ops.chop_rows(x, q, c0, [[-0.1], [0.5]], ok_d)),
            (V, 'dur must lie', lambda: ops.chop_rows(x, q, c0, ok_u, [[1], [-1]])),
            (V, 'dur must be integers', lambda: ops.chop_rows(x, q, c0, ok_u, [[1.5], [1.0]])),
            (V, 'dur must hold', lambda: ops.chop_rows(x, q, c0, ok_u, [[1, 1], [1, 1]])),
            (V, '65535 rows', lambda: ops.chop_rows(big, q, c0, ok_u, ok_d)),
            (Ty, 'bank must be', lambda: ops.fir_rows(x, bank.float(), K, [0, 0])),
            (Ty, 'bank must be', lambda: ops.fir_rows(x, bank[0], K, [0, 0])),
            (V, 'Kmax = 2049', lambda: ops.fir_rows(
                x, torch.zeros(1, 2050, device='cuda', dtype=torch.float64), K[:1], [0, 0])),
            (Ty, 'K must be', lambda: ops.fir_rows(x, bank, K[:2], [0, 0])),
            (Ty, 'K must be', lambda: ops.fir_rows(x, bank, K.long(), [0, 0])),
            (V, 'ids must hold', lambda: ops.fir_rows(x, bank, K, [0])),
            (V, 'ids must be integers', lambda: ops.fir_rows(x, bank, K, [0.0, 1.0])),
            (V, 'device ids', lambda: ops.fir_rows(x, bank, K, torch.zeros(2, device='cuda'))),
            (Ty, 'out_dtype', lambda: ops.fir_rows(x, bank, K, [0, 0], out_dtype=torch.int16)),
            (V, '65535 rows', lambda: ops.fir_rows(big, bank, K, [0] * 65536))):
        with pytest.raises(exc, match=msg):
            call()


# ---- Distort ------------------------------------------------------------------------------------

def _redo_row(kind, sub, j, wave, prev, band):
    """Row j of one kind's rows again, on its own, through the public ops from the recorded draws."""
    from segan_pytorch_amd import ops
    w, p = wave[None].contiguous(), prev[None].contiguous()
    if kind == 'clip':
        y, i = ops.clip_rows(w, sub['factors'][j:j + 1], None, p)
        return y[0], i['prev'][0], i['status'][0]
    if kind == 'chop':
        level = ops.asl_p56_stages(w, 16000, 16)
        y, i = ops.chop_rows(w, level['q'], level['c0'], sub['u'][j:j + 1], sub['dur'][j:j + 1])
        return y[0], prev, i['status'][0]
    bank, K = band.data(wave.device)
    y, i = ops.fir_rows(w, bank, K, sub['ids'][j:j + 1], None, p)
    return y[0], i['prev'][0], i['status'][0]


def test_distort_apply_draws_and_rows():
    from segan_pytorch_amd import augment as A
    rows, T = 9, 16384
    x = np.stack([GA.speech_like(T, 16000, 80 + r) for r in range(rows)])
    prev = (np.arange(rows, dtype=np.float32) - 4) / 8
    xd, pd = _dev(x), _dev(prev)
    clip, chop, band = A.Clip(), A.Chop(), A.BandLimit()
    d = A.Distort([clip, chop, band], seed=5)
    out, info = d.apply(xd, generator=np.random.default_rng(17), prev=pd)
    g = np.random.default_rng(17)
    code = g.integers(3, size=rows)
    assert set(code) == {0, 1, 2} and info['kinds'].tolist() == [A.DISTORT_KINDS[c] for c in code]
    n = [int((code == c).sum()) for c in range(3)]
    assert np.array_equal(info['clip']['factors'], clip.draw(g, n[0]))
    u, dur = chop.draw(g, n[1])
    assert np.array_equal(info['chop']['u'], u) and np.array_equal(info['chop']['dur'], dur)
    assert np.array_equal(info['bandlimit']['ids'], band.draw(g, n[2]))
    for c, kind in enumerate(A.DISTORT_KINDS):
        idx = np.nonzero(code == c)[0]
        assert info[kind]['index'].tolist() == idx.tolist()
        for j, r in enumerate(idx):
            y, p, st = _redo_row(kind, info[kind], j, xd[r], pd[r], band)
            assert torch.equal(out[r], y) and torch.equal(info['prev'][r], p)
            assert int(info['status'][r]) == int(st) == 0
            assert not torch.equal(out[r], xd[r])
    # against the oracle, one row of each kind
    r = int(np.nonzero(code == 0)[0][0])
    o = D.clip(x[r], info['clip']['factors'][0], None, prev[r])
    assert _same(_np(out[r]), o['y']) and float(info['prev'][r]) == float(o['prev'])
    r = int(np.nonzero(code == 2)[0][0])
    K, h = D.lowpass(info['bandlimit']['cutoffs'][0])
    yo, po = D.fir(x[r], h, None, prev[r])
    assert _same(_np(out[r]), yo.astype(np.float32)) and float(info['prev'][r]) == float(np.float32(po))
    # repeatable from the object's seed; a 1-D numpy array through __call__
    a, _ = A.Distort([clip, chop, band], seed=5).apply(xd, prev=pd)
    b, _ = A.Distort([clip, chop, band], seed=5).apply(xd, prev=pd)
    assert torch.equal(a, b)
    for obj in (A.Clip(seed=1), A.Chop(seed=1), A.BandLimit(seed=1), A.Distort([A.Clip()], seed=1)):
        w = obj(x[0])
        assert isinstance(w, torch.FloatTensor) and w.shape == (T,) and not w.is_cuda
        assert not torch.equal(w, torch.from_numpy(x[0]))


# ---- the loader ---------------------------------------------------------------------------------

T_SLICE = 16384


@pytest.fixture(scope='module')
def shard(tmp_path_factory):
    from segan_pytorch_amd.datasets import PCMShardDataset, build_pcm_shard
    d = tmp_path_factory.mktemp('distort_shard')
    cd, nd = d / 'clean', d / 'noisy'
    cd.mkdir()
    nd.mkdir()
    rng = np.random.default_rng(23)
    for i, n in enumerate((41000, 33000)):
        c = np.rint(GA.speech_like(n, 16000, 90 + i).astype(np.float64) * 40000).astype(np.int16)
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


def test_loader_rows_recomposed_from_the_recorded_draws(shard):
    """Distortion on most items, noise on about half.  Per item, from the recorded draws and
    through the public ops on that item alone: the distorted wave (the sample before the slice
    takes part, zero where the slice starts its wav), the noise mixed into it at the level taken
    on it, and the pre-emphasis.  A batched row equals its own call bit for bit, so the loader's
    noisy row must equal the recomposed one exactly."""
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    noises = A.NoiseBank(GA.noise_bank())
    band = A.BandLimit()
    ld = _loader(shard, additive=A.Additive(noises, seed=1), additive_prob=0.5, additive_seed=111,
                 record_additive=True, distort=A.Distort([A.Clip(), A.Chop(), band], seed=2),
                 distort_prob=0.8, distort_seed=[111, 2], record_distort=True)
    got = _batches(ld)
    plain = _batches(_loader(shard))
    addonly = _loader(shard, additive=A.Additive(noises, seed=1), additive_prob=0.5,
                      additive_seed=111, record_additive=True)
    _batches(addonly)
    assert len(got) == len(plain) == 2
    seen, n_both, n_plain = set(), 0, 0
    for k, ((names, clean, noisy, _), (pn, pc, py, _)) in enumerate(zip(got, plain)):
        assert torch.equal(clean, pc)
        rd, ra, ra0 = ld.distort_records[k], ld.additive_records[k], addonly.additive_records[k]
        for key in ('index', 'noise_ids', 'snrs', 'starts'):      # the additive stream stays put
            assert np.array_equal(ra[key], ra0[key]), key
        dsel, asel = rd['index'].tolist(), ra['index'].tolist()
        B = len(names)
        pcm = np.stack([np.array(shard.data[4 * k + r]) for r in range(B)])
        first = shard._first[4 * k:4 * k + B]
        first_d = _dev(first)
        dry = ((2.0 / 65535.0) * (pcm[:, 0].astype(np.float64) - 32767.0) + 1.0).astype(np.float32)
        for r in range(B):
            wave, prev = _dev(dry[r, 1:]), _scalar(0.0 if first[r] else dry[r, 0])
            want = pn[r]
            if r in dsel:
                j = dsel.index(r)
                kind = rd['kinds'][j]
                assert torch.equal(rd['wave'][j], wave) and torch.equal(rd['wave_prev'][j], prev)
                jj = rd[kind]['index'].tolist().index(j)
                wave, prev, st = _redo_row(kind, rd[kind], jj, wave, prev, band)
                assert torch.equal(rd['out'][j], wave) and int(st) == 0
                want += '_' + kind
                seen.add(kind)
            elif r in asel:
                prev = _scalar(dry[r, 0])      # additive alone takes the stored sample as it is
            if r in asel:
                j = asel.index(r)
                assert torch.equal(ra['wave'][j], wave) and torch.equal(ra['wave_prev'][j], prev)
                level = ops.asl_p56(wave[None].contiguous())
                mixed, mi = ops.additive_mix(wave[None].contiguous(), noises.data('cuda'),
                                             ra['abs_starts'][j:j + 1], ra['snrs'][j:j + 1],
                                             level['asl_ms'], None, prev[None].contiguous())
                wave, prev = mixed[0], mi['prev'][0]
                want += '_additive'
                n_both += r in dsel
            assert names[r] == want
            if r in dsel or r in asel:
                row = torch.empty(1, T_SLICE, device='cuda')
                ops.preemph_rows(wave[None].contiguous(), prev[None].contiguous(),
                                 first_d[r:r + 1].contiguous(), row, 0.95)
                assert torch.equal(noisy[r], row[0].cpu()), (k, r)
                assert not torch.equal(noisy[r], py[r])
            else:
                assert torch.equal(noisy[r], py[r])
                n_plain += 1
    assert seen == {'clip', 'chop', 'bandlimit'} and n_both >= 1, (seen, n_both, n_plain)


def test_loader_three_stages_recomposed_from_the_recorded_draws(shard):
    """Reverb, distortion and noise together.  Per item, from the recorded draws and through the
    public ops on that item alone, in the loader's order: the reverberant wave, the distorted wave,
    the noise mixed into what those left, and the pre-emphasis with the preceding sample as the
    stages transformed it.  A batched row equals its own call bit for bit for every op involved, so
    the loader's noisy row must equal the recomposed one exactly.  The first batch holds an item
    that every stage selected (each takes over the rows of the one before), one with reverb and
    noise (noise on a row that the distort stage kept from the reverb stage), one with distortion
    alone and one with reverb and distortion."""
    from segan_pytorch_amd import augment as A
    from segan_pytorch_amd import ops
    noises = A.NoiseBank(GA.noise_bank())
    rbank = A.RIRBank([GR.rir_bank()[i] for i in (6, 10, 11, 7)])      # 300, 4099, 100, 300 taps
    band = A.BandLimit()
    ld = _loader(shard, reverb=A.Reverb(rbank), reverb_prob=0.6, reverb_seed=2, record_reverb=True,
                 distort=A.Distort([A.Clip(), A.Chop(), band]), distort_prob=0.6, distort_seed=12,
                 record_distort=True, additive=A.Additive(noises), additive_prob=0.5,
                 additive_seed=3, record_additive=True)
    got = _batches(ld)
    plain = _batches(_loader(shard))
    assert len(got) == len(plain) == 2
    seen = []
    for k, ((names, clean, noisy, _), (pn, pc, py, _)) in enumerate(zip(got, plain)):
        assert torch.equal(clean, pc)
        rr, rd, ra = ld.reverb_records[k], ld.distort_records[k], ld.additive_records[k]
        rsel, dsel, asel = ([] if rec is None else rec['index'].tolist() for rec in (rr, rd, ra))
        B = len(names)
        pcm = np.stack([np.array(shard.data[4 * k + r]) for r in range(B)])
        first = shard._first[4 * k:4 * k + B]
        first_d = _dev(first)
        dry = ((2.0 / 65535.0) * (pcm[:, 0].astype(np.float64) - 32767.0) + 1.0).astype(np.float32)
        for r in range(B):
            wave, prev = _dev(dry[r, 1:]), _scalar(0.0 if first[r] else dry[r, 0])
            want = pn[r]
            if r in rsel:
                j = rsel.index(r)
                assert torch.equal(rr['wave'][j], wave) and torch.equal(rr['wave_prev'][j], prev)
                wet, wi = ops.reverb_rows(wave[None].contiguous(), rbank, rr['rir_ids'][j:j + 1],
                                          None, prev[None].contiguous())
                wave, prev = wet[0], wi['prev'][0]
                assert torch.equal(rr['wet'][j], wave) and int(wi['status'][0]) == 0
                want += '_reverb'
            if r in dsel:
                j = dsel.index(r)
                kind = rd['kinds'][j]
                assert torch.equal(rd['wave'][j], wave) and torch.equal(rd['wave_prev'][j], prev)
                jj = rd[kind]['index'].tolist().index(j)
                wave, prev, st = _redo_row(kind, rd[kind], jj, wave, prev, band)
                assert torch.equal(rd['out'][j], wave) and int(st) == 0
                want += '_' + kind
            if r in asel:
                if r not in rsel and r not in dsel:
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
            if r in rsel or r in dsel or r in asel:
                row = torch.empty(1, T_SLICE, device='cuda')
                ops.preemph_rows(wave[None].contiguous(), prev[None].contiguous(),
                                 first_d[r:r + 1].contiguous(), row, 0.95)
                assert torch.equal(noisy[r], row[0].cpu()), (k, r)
                assert not torch.equal(noisy[r], py[r])
            else:
                assert torch.equal(noisy[r], py[r])
            seen.append((r in rsel, r in dsel, r in asel))
    # (reverb, distort, additive) of the first batch's items: the four combinations above
    assert seen[:4] == [(True, True, True), (True, False, True), (False, True, False),
                        (True, True, False)], seen


def test_loader_without_distort_is_unchanged(shard):
    from segan_pytorch_amd import augment as A
    noises = A.NoiseBank(GA.noise_bank())
    kw = dict(additive_prob=0.5, additive_seed=7)
    a = _batches(_loader(shard, additive=A.Additive(noises, seed=1), **kw))
    b = _batches(_loader(shard, additive=A.Additive(noises, seed=1), distort=None, distort_prob=0.3,
                         distort_seed=5, **kw))
    c = _batches(_loader(shard, additive=A.Additive(noises, seed=1),
                         distort=A.Distort([A.Clip()]), distort_prob=0.0, distort_seed=5, **kw))
    for other in (b, c):
        assert len(a) == len(other) == 2
        for u, v in zip(a, other):
            assert u[0] == v[0] and all(torch.equal(p, q) for p, q in zip(u[1:], v[1:]))


# ---- train.py -----------------------------------------------------------------------------------

CHILD = '''
import os, sys
sys.path.insert(0, {root!r})
import train
from segan_pytorch_amd import datasets
prep = datasets.PCMShardLoader._prep
def show(self, item):
    batch = prep(self, item)
    print('NAMES', ' '.join(batch[0]), flush=True)
    return batch
datasets.PCMShardLoader._prep = show
opts = train.build_parser().parse_args(sys.argv[1:])
opts.bias = not opts.no_bias
os.makedirs(opts.save_path, exist_ok=True)
train.main(opts)
'''


@pytest.mark.parametrize('extra', [[], ['--wsegan', '--opt', 'adam']], ids=['segan', 'wsegan'])
def test_train_with_distort(tmp_path, extra):
    """A short train.py run at batch 4 with --distort clip chop bandlimit --distort_prob 0.7 in a
    fresh child process: it runs, and the names carry the kinds."""
    from segan_pytorch_amd.datasets import build_pcm_shard
    cd, nd = tmp_path / 'clean', tmp_path / 'noisy'
    for d in (cd, nd):
        d.mkdir()
    for i in range(3):
        c = np.rint(GA.speech_like(6000, 16000, 40 + i).astype(np.float64) * 30000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000, c)
    assert build_pcm_shard(str(cd), str(nd), str(tmp_path / 'sh'), slice_size=1024, stride=0.5) >= 8
    ck = str(tmp_path / 'ckpt')
    cmd = [sys.executable, '-c', CHILD.format(root=ROOT), '--save_path', ck, '--pcm_shard',
           str(tmp_path / 'sh'), '--distort', 'clip', 'chop', 'bandlimit', '--distort_prob', '0.7',
           '--chop_durs', '0.005', '0.02', '--batch_size', '4', '--epoch', '1', '--save_freq', '1',
           '--no_train_gen', '--genc_fmaps', '8', '16', '32', '--denc_fmaps', '8', '16', '32',
           '--genc_poolings', '4', '4', '4', '--denc_poolings', '4', '4', '4', '--z_dim', '32',
           '--slice_size', '1024', '--num_workers', '0'] + extra
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'btime' in out.stdout and 'nan' not in out.stdout.lower()
    names = [n for ln in out.stdout.splitlines() if ln.startswith('NAMES') for n in ln.split()[1:]]
    tails = [n.rsplit('_', 1)[1] if '_' in n else '' for n in names]
    kinds = {'clip', 'chop', 'bandlimit'}
    assert len(names) >= 8 and set(tails) >= kinds, names
    assert all(t in kinds or n in ('u0', 'u1', 'u2') for t, n in zip(tails, names)), names
    assert any(n in ('u0', 'u1', 'u2') for n in names)      # --distort_prob 0.7 leaves some alone
