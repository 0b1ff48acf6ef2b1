"""The reverberation augmentation without a GPU: the float64 oracle
(scripts/reverb_oracle.py) against a literal double loop and against scipy's fftconvolve, the
fixture tests/golden/reverb.pt (recipe scripts/make_golden_reverb.py), RIRBank's normalisation, the
loader's selection / naming / draw logic with the device ops replaced by host stand-ins, the
train.py flags and the C ABI."""
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
import make_golden_reverb as G  # noqa: E402
import reverb_oracle as R  # noqa: E402


@pytest.fixture(scope='module')
def rfx():
    return load_golden('reverb.pt')


@pytest.fixture(scope='module')
def bank():
    return [R.normalise(h) for h in G.rir_bank()]


# ---- the oracle ---------------------------------------------------------------------------------

def literal(x, h, d, n, prev):
    """y[m] = sum_k h[k] x[m + d - k], m = -1 .. n-1, as two loops."""
    def at(i):
        if i == -1:
            return 0.0 if prev is None else float(prev)
        return float(x[i]) if 0 <= i < n else 0.0
    out = []
    for m in range(-1, n):
        acc = 0.0
        for k in range(len(h)):
            acc += float(h[k]) * at(m + d - k)
        out.append(acc)
    return np.array(out[1:] + [0.0] * (len(x) - n)), out[0]


@pytest.mark.parametrize('L', [1, 2, 5])
@pytest.mark.parametrize('prev', [None, 0.7])
def test_oracle_equals_the_double_loop(L, prev):
    rng = np.random.default_rng(10 * L)
    T = 9
    x = rng.standard_normal(T)
    for d in sorted({0, L - 1}):
        h = rng.standard_normal(L)
        for n in (T, 4, 1, 0):
            y, p = R.reverb(x, h, d, n, prev)
            yl, pl = literal(x, h, d, n, prev)
            assert np.abs(y - yl).max() <= 1e-14 and abs(p - pl) <= 1e-14, (L, d, n)
            assert not y[n:].any()
    # d = 0, L = 1, h = [1]: the identity, and y[-1] = prev
    y, p = R.reverb(x, [1.0], 0, None, prev)
    assert np.array_equal(y, x) and p == (0.0 if prev is None else prev)


def test_fixture_cases_and_fftconvolve(rfx, bank):
    assert rfx['cases'] == G.CASES and rfx['bank'] == list(G.BANK) and rfx['batch'] == G.BATCH
    assert [G.sha(h) for h, _ in bank] == rfx['rir_sha']
    assert {rc['T'] for rc in G.CASES.values()} == {1, 127, 128, 129, 1000, 16384}
    assert {rc['taps'] for rc in G.BANK} >= {1, 2, 128, 129, 300, 4099}
    parts = {-(-G.BANK[r]['taps'] // 128) for r in G.BATCH['rirs'] if r < len(G.BANK)}
    assert parts >= {1, 3, 33} and max(G.BATCH['rirs']) >= len(G.BANK)
    for name, rc in G.CASES.items():
        x, length, prev = G.case_signal(rc)
        assert G.sha(x) == rfx['sha'][name], name
        h, d = bank[rc['rir']]
        y, p = R.reverb(x, h, d, length, prev)
        s = R.scale(x, h, d, length, prev)
        assert s == rfx['scale'][name]
        yf, pf = G.against_fft(x, h, d, length, prev)
        assert max(np.abs(y - yf).max(), abs(p - pf)) <= 1e-13 * s, name
        want = rfx['y'][name].numpy()
        assert np.abs(G.stored(y) - want).max() <= 1e-13 * s, name
        assert abs(p - rfx['prev_out'][name]) <= 1e-13 * s, name
        if 'n0' in rc:      # an impulse probe shows the response itself, tap by tap
            n = rc.get('length', rc['T'])
            n0 = n - 1 if rc['n0'] == 'last' else rc['n0']
            for m in range(n):
                k = m + d - n0
                assert y[m] == (h[k] if 0 <= k < len(h) else 0.0), (name, m)
    xb, pb = G.batch_signal()
    assert G.sha(xb) == rfx['sha']['batch']


# ---- RIRBank ------------------------------------------------------------------------------------

def test_rir_bank_normalises_on_the_host(tmp_path):
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import Reverb, RIRBank
    h0 = np.array([0.1, -0.5, 0.25, 0.5])            # negative peak, first occurrence of |0.5|
    h1 = np.concatenate((np.zeros(5), [0.3], 0.01 * np.ones(300)))
    h2 = np.array([3, -32768, 100], dtype=np.int16)
    b = RIRBank([h0, h1, torch.from_numpy(h2)], max_taps=200)
    assert len(b) == 3 and b.delays.tolist() == [1, 5, 1] and b.taps.tolist() == [4, 200, 3]
    for h, d in zip(b.rirs, b.delays):
        assert h.dtype == np.float32 and h[d] == np.float32(1.0)
    assert np.array_equal(b.rirs[0], (h0 / -0.5).astype(np.float32))      # divides through
    assert b.rirs[0][3] == -1.0 and np.abs(b.rirs[0]).max() == 1.0
    assert np.array_equal(b.rirs[1], (h1[:200] / 0.3).astype(np.float32))
    assert np.array_equal(b.rirs[2], (h2.astype(np.float64) / -32768.0).astype(np.float32))
    assert np.array_equal(R.normalise(h1, 200)[0], b.rirs[1]) and R.normalise(h1, 200)[1] == 5
    P = ops.REVERB_P
    assert b.partitions.tolist() == [1, 2, 1] and b.offsets.tolist() == [0, 1, 3, 4]
    pad = b.padded()
    assert pad.shape == (4, P) and np.array_equal(pad.reshape(-1)[P:P + 200], b.rirs[1])
    assert not pad.reshape(-1)[P + 200:3 * P].any()
    # the peak beyond max_taps is cut off with the tail; what is left decides
    late = np.concatenate(([0.0, 0.2], np.zeros(10), [5.0]))
    assert RIRBank([late], max_taps=12).delays.tolist() == [1]
    for bad in (np.zeros(7), np.concatenate((np.zeros(12), [1.0])), np.zeros(0)):
        with pytest.raises(ValueError, match='no non-zero tap'):
            RIRBank([bad], max_taps=12)
    with pytest.raises(ValueError, match='No impulse responses'):
        RIRBank([])
    with pytest.raises(TypeError, match='float or int16'):
        RIRBank([np.arange(4)])
    with pytest.raises(RuntimeError, match='MI355X'):
        b.data('cpu')
    # from_dir: the wav reader of NoiseBank.from_dir (int16 / 32768, channels averaged), sorted
    st = np.stack([h2, h2[::-1]], axis=1)
    wavfile.write(str(tmp_path / 'b.wav'), 16000, h2)
    wavfile.write(str(tmp_path / 'a.wav'), 48000, st)
    d = RIRBank.from_dir(str(tmp_path))
    assert [os.path.basename(f) for f in d.files] == ['a.wav', 'b.wav']
    assert np.array_equal(d.rirs[1], b.rirs[2]) and d.delays.tolist() == [1, 1]
    assert np.array_equal(d.rirs[0], R.normalise(st.astype(np.float32).mean(axis=1) / 32768.0)[0])
    with pytest.raises(ValueError, match='No impulse responses'):
        RIRBank.from_dir(str(tmp_path / 'none'))
    rv = Reverb(b, seed=3)
    assert rv.bank is b
    ids = rv.draw(np.random.default_rng(3), 50)
    assert ids.min() == 0 and ids.max() == 2
    assert np.array_equal(ids, Reverb(b).draw(np.random.default_rng(3), 50))
    with pytest.raises(ValueError, match='rir ids'):
        rv.draw(rv.rng, 2, [0, 3])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='MI355X'):
            rv(np.zeros(10))
        with pytest.raises(RuntimeError, match='MI355X'):
            rv.apply(torch.zeros(2, 8))


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
    for i in range(2):
        c = (rng.standard_normal(200) * 3000).astype(np.int16)
        wavfile.write(str(cd / 'u{}.wav'.format(i)), 16000, c)
        wavfile.write(str(nd / 'u{}.wav'.format(i)), 16000, c)
    assert build_pcm_shard(str(cd), str(nd), str(tmp_path / 'sh'), slice_size=T_SLICE,
                           stride=0.5) >= 8
    return PCMShardDataset(str(tmp_path / 'sh'))


def run_loader(shard, **kw):
    from segan_pytorch_amd.datasets import PCMShardLoader
    ld = PCMShardLoader(shard, 4, 0.95, 'cpu', num_workers=0, record_additive=True,
                        record_reverb=True, **kw)
    out = [ld._prep(shard.gather(range(k, k + 4))) for k in (0, 4)]
    return out, ld


def test_loader_selects_names_and_keeps_the_additive_draws(shard, monkeypatch):
    host_ops(monkeypatch)
    plain, _ = run_loader(shard)
    none, ld0 = run_loader(shard, reverb=None, reverb_prob=0.3, reverb_seed=9)
    assert ld0.reverb_records == []
    add_only, lda = run_loader(shard, additive=host_additive(), additive_prob=0.5, additive_seed=3)
    rv = HostReverb()
    both, ldb = run_loader(shard, additive=host_additive(), additive_prob=0.5, additive_seed=3,
                           reverb=rv, reverb_prob=0.5, reverb_seed=8)
    for a, b in zip(plain, none):
        assert a[0] == b[0] and all(torch.equal(u, v) for u, v in zip(a[1:], b[1:]))
    n_both = n_rev_only = n_add_only = 0
    for k in range(2):
        names, clean, noisy, _ = both[k]
        pn, pc, py, _ = plain[k]
        an = add_only[k][0]
        assert torch.equal(clean, pc)      # clean is never touched
        ra, rb, rr = lda.additive_records[k], ldb.additive_records[k], ldb.reverb_records[k]
        # the additive selection and draws (ids, SNRs, starts) do not move when reverb is on
        for key in ('index', 'noise_ids', 'snrs', 'starts'):
            assert np.array_equal(ra[key], rb[key]), key
        asel, rsel = set(rb['index'].tolist()), set(rr['index'].tolist())
        for i in range(4):
            want = pn[i] + ('_reverb' if i in rsel else '') + ('_additive' if i in asel else '')
            assert names[i] == want
            assert an[i] == pn[i] + ('_additive' if i in asel else '')
        pcm = torch.from_numpy(np.stack([np.array(shard.data[4 * k + i]) for i in range(4)]))
        w = ((2.0 / 65535.0) * (pcm[:, 0].double() - 32767.0) + 1.0).float()
        first = shard._first[4 * k:4 * k + 4]
        call = rv.calls[k]
        for j, i in enumerate(rr['index'].tolist()):      # the dry clean wave goes into the reverb
            assert torch.equal(call['wave'][j], w[i, 1:])
            assert call['prev'][j] == (0.0 if first[i] else w[i, 0])
        for i in range(4):
            dry, dprev = w[i, 1:], w[i, 0]
            if i in rsel:
                j = rr['index'].tolist().index(i)
                wet, wprev = dry * 2, call['prev'][j] * 2 + 1
            if i in asel and i in rsel:      # noise is mixed into the reverberant wave
                ja = rb['index'].tolist().index(i)
                assert torch.equal(rb['wave'][ja], wet) and rb['wave_prev'][ja] == wprev
                assert torch.equal(noisy[i], (wet + 7) + 100 * (wprev + 7))
                n_both += 1
            elif i in asel:
                ja = rb['index'].tolist().index(i)
                assert torch.equal(rb['wave'][ja], dry) and rb['wave_prev'][ja] == dprev
                assert torch.equal(noisy[i], (dry + 7) + 100 * (dprev + 7))
                n_add_only += 1
            elif i in rsel:                  # the reverberant wave through the pre-emphasis
                assert torch.equal(noisy[i], wet + 100 * wprev)
                n_rev_only += 1
            else:
                assert torch.equal(noisy[i], py[i])
    assert n_both and n_rev_only and n_add_only
    # reverb alone, every item; its draws come from its own seeded generator
    r1, r2 = HostReverb(), HostReverb()
    one, ld1 = run_loader(shard, reverb=r1, reverb_seed=8)
    two, _ = run_loader(shard, reverb=r2, reverb_seed=8)
    other, ldo = run_loader(shard, reverb=HostReverb(), reverb_seed=9)
    assert all(n.endswith('_reverb') for b in one for n in b[0]) and ld1.additive_records is not None
    assert all(np.array_equal(a['ids'], b['ids']) for a, b in zip(r1.calls, r2.calls))
    assert any(not np.array_equal(a['rir_ids'], b['rir_ids'])
               for a, b in zip(ld1.reverb_records, ldo.reverb_records))
    zero, ldz = run_loader(shard, reverb=HostReverb(), reverb_prob=0.0, reverb_seed=8)
    assert ldz.reverb_records == [None, None]
    for a, b in zip(plain, zero):
        assert a[0] == b[0] and torch.equal(a[2], b[2])


def test_loader_checks_the_probability():
    from segan_pytorch_amd.datasets import PCMShardLoader
    with pytest.raises(ValueError, match='reverb_prob'):
        PCMShardLoader(None, 2, 0.95, 'cpu', reverb=object(), reverb_prob=-0.1)


# ---- train.py flags -----------------------------------------------------------------------------

def test_train_flags_parse_and_go_with_pcm_shard():
    import train
    p = train.build_parser()
    d = p.parse_args([])
    assert d.reverb_rirs is None and d.reverb_prob == 1.0 and d.reverb_max_taps == 16384
    assert d.reverb_resample is False and train.check_reverb_flags(d) is False
    o = p.parse_args(['--pcm_shard', 'sh', '--reverb_rirs', 'dir', '--reverb_prob', '0.25',
                      '--reverb_max_taps', '4000', '--reverb_resample'])
    assert o.reverb_prob == 0.25 and o.reverb_max_taps == 4000 and o.reverb_resample is True
    assert train.check_reverb_flags(o) is True and train.check_additive_flags(o) is False
    o = p.parse_args(['--pcm_shard', 'sh', '--reverb_rirs', 'dir', '--additive_noises', 'n'])
    assert train.check_reverb_flags(o) is True and train.check_additive_flags(o) is True
    for bad, msg in ((['--reverb_rirs', 'dir'], 'only together with --pcm_shard'),
                     (['--reverb_rirs', 'dir', '--synthetic', '8'], 'only together with'),
                     (['--pcm_shard', 'sh', '--reverb_prob', '0.5'], 'need --reverb_rirs'),
                     (['--pcm_shard', 'sh', '--reverb_max_taps', '100'], 'need --reverb_rirs'),
                     (['--pcm_shard', 'sh', '--reverb_resample'], 'needs --reverb_rirs'),
                     (['--pcm_shard', 'sh', '--reverb_rirs', 'd', '--reverb_prob', '1.5'],
                      'must lie in 0 .. 1'),
                     (['--pcm_shard', 'sh', '--reverb_rirs', 'd', '--reverb_max_taps', '0'],
                      'must be positive')):
        with pytest.raises(SystemExit, match=msg):
            train.check_reverb_flags(p.parse_args(bad))
        with pytest.raises(SystemExit, match=msg):      # before anything touches a device
            train.main(p.parse_args(bad))
    assert '--reverb_rirs' in train.__doc__ and '--reverb_max_taps' in train.__doc__


# ---- C ABI --------------------------------------------------------------------------------------

REVERB_SYMBOLS = ('segan_reverb_dims', 'segan_reverb_basis', 'segan_reverb_bank',
                  'segan_reverb_stage', 'segan_reverb_forward', 'segan_reverb_fdl',
                  'segan_reverb_inverse', 'segan_reverb_finish', 'segan_reverb_rows')


def test_header_lib_and_abi_agree():
    import ctypes
    from segan_pytorch_amd import _lib, ops
    assert H.macro('SEGAN_ABI_VERSION') == 17
    assert H.macro('SEGAN_REVERB_P') == ops.REVERB_P
    assert _lib.ABI_VERSION == 17
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in REVERB_SYMBOLS:
        assert len(H.args(name)) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name) and name in doc
    # host-only sizing, and arguments validated before any launch
    P = ops.REVERB_P
    dims = (ctypes.c_int64 * 8)()
    assert lib.segan_reverb_dims(300, 16384, 0, 16384, dims) == 0
    assert list(dims)[:4] == [P, 130, 300 * 130, 128]
    assert dims[4] == (dims[2] + 1) * P and dims[5] == dims[2] * 2 * P and dims[6] == dims[2] * P
    assert dims[7] == dims[4] + 2 * dims[5] + dims[6]
    assert ops.reverb_dims(1, 1, 0)['blocks'] == 3 and ops.reverb_dims(1, 1, 0)['frames'] == 32
    assert ops.reverb_dims(2, 128, 127)['blocks'] == 3      # x[127] + 127 ends block 2
    assert ops.reverb_dims(2, 129, 127)['blocks'] == 4
    assert ops.reverb_dims(2, 129, 4098)['blocks'] == (128 + 128 + 4098) // P + 1
    assert lib.segan_reverb_dims(0, 16, 0, 1, dims) == -1 and b'reverb_dims' in lib.segan_last_error()
    assert lib.segan_reverb_dims(1, 16, 5, 5, dims) == -1      # the delay is a tap of the RIR
    buf = torch.zeros(64)
    q = buf.data_ptr()
    assert lib.segan_reverb_rows(q, None, None, q, 1, q, q, 1, q, q, 1, 16, 0, None, 0, q, q, q,
                                 None) == -1
    assert lib.segan_reverb_rows(q, None, None, q, 1, q, q, 1, q, q, 1, 16, 0, q, 10, q, q, q,
                                 None) == -1
    assert b'workspace' in lib.segan_last_error()
    assert lib.segan_reverb_fdl(q, q, 1, q, q, 1, q, 1, 16, 2, 32, None) == -1     # too few blocks
    assert b'segan_reverb_dims' in lib.segan_last_error()
    assert lib.segan_reverb_stage(None, None, None, q, 1, 16, 3, 32, None) == -1
