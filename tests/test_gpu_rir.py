"""Room impulse responses by the image-source method on the MI355X (ops.rir_shoebox / rir_stages,
augment.RIRBank.synthetic) against the numpy oracle scripts/rir_oracle.py and its fixture
tests/golden/rir.pt.

Decisions.  The definition has none: the window vanishes at its edge, so an image that one side
takes and the other leaves contributes nothing.  The image count of a row is a decision, floor(tau)
against the row's end; scripts/make_golden_rir.py refuses a row where an image is closer than 1e-9
samples to it (the closest of the fixture is 5.8e-4 samples away), so the counts are compared
exactly, with no exemption.

Tolerance: every row within 100 x the movement of the oracle between float64 and
numpy.longdouble, as the fixture recorded it per row (1.4e-15 to 4.9e-14 of max |h|, so bounds of
1.4e-13 to 4.9e-12 of max |h|; zero for the row that ends before the direct path arrives).

Measured on an MI355X (each test prints its figures): the figures are in README.md beside the
bounds.  The tolerances stay as asserted."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_rir as GR  # noqa: E402
import reverb_oracle as RV  # noqa: E402

pytestmark = pytest.mark.gpu

REVERB_TOL = 1e-4         # tests/test_gpu_reverb.py's


@pytest.fixture(scope='module')
def rfx():
    return load_golden('rir.pt')


def _bits(t):
    return t.contiguous().view(torch.int64).cpu()


def _run(c, stages=True, T=None, lengths='own'):
    from segan_pytorch_amd import ops
    g = c['geom'].numpy()
    T = c['T'] if T is None else T
    if lengths == 'own':
        lengths = None if c['length'] == c['T'] else [c['length']]
    fn = ops.rir_stages if stages else ops.rir_shoebox
    return fn(g[None, 0:3], g[None, 3:6], g[None, 6:9], g[None, 9:15], T, srate=c['srate'],
              lengths=lengths)


@pytest.mark.parametrize('name', list(GR.ROWS))
def test_rows_match_the_oracle(rfx, name):
    c = rfx['rows'][name]
    assert np.array_equal(c['geom'].numpy(), GR.geom_of(GR.ROWS[name]))
    out = _run(c)
    got, want = out['h'][0].cpu().numpy(), c['h'].numpy()
    assert got.shape == want.shape and got.dtype == np.float64
    err = float(np.abs(got - want).max())
    peak = c['peak'] if c['peak'] else 1.0
    print('{}: images {} err/peak {:.3e} bound {:.3e}'.format(
        name, int(out['images'][0]), err / peak, 100 * c['move'] / peak))
    assert not got[c['length']:].any()
    assert err <= 100 * c['move']
    assert int(out['images'][0]) == c['images']
    if name == 'T1':
        assert c['images'] == 0 and not got.any()


def test_a_batch_equals_its_rows_bit_for_bit(rfx):
    from segan_pytorch_amd import ops
    names = ['T2048', 'small_live', 'cube_centre', 'dead', 'near', 'masked']
    rows = [rfx['rows'][n] for n in names]
    T = 640
    g = np.stack([c['geom'].numpy() for c in rows])
    lens = [min(c['length'], T) for c in rows]
    both = ops.rir_stages(g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:15], T, lengths=lens)
    again = ops.rir_stages(g[:, 0:3], g[:, 3:6], g[:, 6:9], g[:, 9:15], T, lengths=lens)
    assert torch.equal(_bits(both['h']), _bits(again['h']))          # two calls of the same input
    assert torch.equal(both['images'].cpu(), again['images'].cpu())
    for i, c in enumerate(rows):
        one = _run(c, T=T, lengths=[lens[i]])
        assert torch.equal(_bits(one['h'][0]), _bits(both['h'][i])), names[i]
        assert int(one['images'][0]) == int(both['images'][i])
        assert both['h'][i].abs().max() > 0


def test_a_prefix_does_not_depend_on_T_or_on_lengths(rfx):
    c = rfx['rows']['T2048']
    full = _run(c, stages=False)
    assert full.shape == (1, 2048)
    for T1 in (255, 256, 257, 700):
        short = _run(c, stages=False, T=T1, lengths=None)
        assert torch.equal(_bits(short[0]), _bits(full[0, :T1])), T1
        cut = _run(c, T=2048, lengths=[T1])
        assert torch.equal(_bits(cut['h'][0, :T1]), _bits(full[0, :T1])), T1
        assert not cut['h'][0, T1:].any()
        assert int(cut['images'][0]) == int(_run(c, T=T1, lengths=None)['images'][0])
    want = rfx['rows']['T255']
    assert int(_run(c, T=255, lengths=None)['images'][0]) == want['images']
    zero = _run(c, T=300, lengths=[0])
    assert not zero['h'].any() and int(zero['images'][0]) == 0


def test_synthetic_bank_end_to_end():
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import RIRBank, Reverb, draw_rooms
    bank = RIRBank.synthetic(4, seed=1, device='cuda', max_taps=2048)
    rooms = draw_rooms(np.random.default_rng(1), 4)
    for k in rooms:
        assert np.array_equal(rooms[k], bank.rooms[k])
    assert len(bank) == 4 and bank.taps.tolist() == np.minimum(
        2048, np.ceil(1.5 * rooms['rt60'] * 16000)).astype(int).tolist()
    dist = np.sqrt(((rooms['src'] - rooms['mic']) ** 2).sum(axis=1))
    direct = np.round(dist * 16000 / 343.0)
    print('delays', bank.delays.tolist(), 'direct paths', direct.tolist())
    assert np.all(np.abs(bank.delays - direct) <= 1)
    for h, d in zip(bank.rirs, bank.delays):
        assert h.dtype == np.float32 and h[d] == 1.0 and np.abs(h).max() == 1.0
    x = np.random.default_rng(2).standard_normal((4, 4096)).astype(np.float32) * 0.1
    ids = [0, 1, 2, 3]
    y, info = ops.reverb_rows(torch.from_numpy(x).cuda(), bank, ids)
    assert info['status'].cpu().tolist() == [0] * 4
    worst = 0.0
    for i in ids:
        h, d = bank.rirs[i], int(bank.delays[i])
        yo, po = RV.reverb(x[i], h, d)
        s = RV.scale(x[i], h, d)
        e = max(float(np.abs(y[i].cpu().numpy().astype(np.float64) - yo).max()),
                abs(float(info['prev'][i]) - po)) / s
        worst = max(worst, e)
    print('reverb through the synthetic bank: E', worst)
    assert worst <= REVERB_TOL
    wet, info = Reverb(bank, seed=0).apply(torch.from_numpy(x).cuda())
    assert wet.shape == (4, 4096) and bool(torch.isfinite(wet).all())


def test_values_are_refused_before_any_launch():
    from segan_pytorch_amd import ops
    ok = dict(room=[5, 4, 3], src=[1, 1, 1], mic=[2, 2, 2], beta=[0.5] * 6, taps=64)
    for bad, msg in ((dict(room=[0.5, 4, 3]), 'not in 1 .. 50'), (dict(room=[51, 4, 3]), '1 .. 50'),
                     (dict(src=[5, 1, 1]), 'strictly inside'), (dict(mic=[2, 0, 2]), 'strictly'),
                     (dict(mic=[1, 1, 1.01]), 'below 0.05'), (dict(beta=[0.5] * 5 + [1.5]), 'beta'),
                     (dict(beta=[-0.1] + [0.5] * 5), 'beta')):
        with pytest.raises(RuntimeError, match='rir: room 0.*' + msg):
            ops.rir_shoebox(**dict(ok, **bad))
    assert ops.rir_shoebox(**ok).shape == (1, 64)


# ---- scripts/synth_rirs.py and train.py ---------------------------------------------------------

CHILD = '''
import os, sys
sys.path.insert(0, {root!r})
import train
from segan_pytorch_amd import augment, datasets
prep = datasets.PCMShardLoader._prep
def show(self, item):
    batch = prep(self, item)
    print('NAMES', ' '.join(batch[0]), flush=True)
    return batch
datasets.PCMShardLoader._prep = show
init = augment.Reverb.__init__
def note(self, rirs, *a, **kw):
    init(self, rirs, *a, **kw)
    print('BANK', ' '.join(os.path.basename(f) for f in self.bank.files), flush=True)
    print('TAPS', ' '.join(str(t) for t in self.bank.taps), flush=True)
augment.Reverb.__init__ = note
opts = train.build_parser().parse_args(sys.argv[1:])
opts.bias = not opts.no_bias
os.makedirs(opts.save_path, exist_ok=True)
train.main(opts)
'''


def test_synth_rirs_writes_a_bank_that_train_reads_beside_reverb_synth(tmp_path):
    """scripts/synth_rirs.py writes two responses and rooms.csv; one step of train.py at batch 2
    with that directory as --reverb_rirs and --reverb_synth 3 beside it: the files' responses come
    first in the bank, the three synthetic ones follow, cut to --reverb_max_taps."""
    import csv
    import subprocess
    from scipy.io import wavfile
    import make_golden_additive as GA
    import synth_rirs as S
    from segan_pytorch_amd import ops
    from segan_pytorch_amd.augment import RIRBank, draw_rooms
    from segan_pytorch_amd.datasets import build_pcm_shard
    rd = tmp_path / 'rirs'
    S.main(S.build_parser().parse_args(['--out', str(rd), '--count', '2', '--seed', '9',
                                        '--max_taps', '700', '--rt60', '0.2', '0.3']))
    assert sorted(os.listdir(str(rd))) == ['rir_0000.wav', 'rir_0001.wav', 'rooms.csv']
    rooms = draw_rooms(np.random.default_rng(9), 2, rt60=(0.2, 0.3))
    with open(str(rd / 'rooms.csv')) as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == S.COLUMNS and len(lines) == 3
    h = ops.rir_shoebox(rooms['room'], rooms['src'], rooms['mic'], rooms['beta'], 700).cpu().numpy()
    for i in range(2):
        rate, w = wavfile.read(str(rd / 'rir_{:04d}.wav'.format(i)))
        assert rate == 16000 and w.dtype == np.float32 and len(w) == 700 == int(lines[i + 1][1])
        assert np.array_equal(w, h[i].astype(np.float32))
        assert [float(v) for v in lines[i + 1][4:7]] == rooms['room'][i].tolist()
    assert RIRBank.from_dir(str(rd)).taps.tolist() == [700, 700]
    cd, nd = tmp_path / 'clean', tmp_path / 'noisy'
    cd.mkdir()
    nd.mkdir()
    c = np.rint(GA.speech_like(1536, 16000, 45).astype(np.float64) * 30000).astype(np.int16)
    wavfile.write(str(cd / 'u0.wav'), 16000, c)
    wavfile.write(str(nd / 'u0.wav'), 16000, c)
    assert build_pcm_shard(str(cd), str(nd), str(tmp_path / 'sh'), slice_size=1024, stride=0.5) == 2
    cmd = [sys.executable, '-c', CHILD.format(root=ROOT), '--save_path', str(tmp_path / 'ckpt'),
           '--pcm_shard', str(tmp_path / 'sh'), '--reverb_rirs', str(rd), '--reverb_synth', '3',
           '--reverb_rt60', '0.2', '0.3', '--reverb_max_taps', '512', '--batch_size', '2',
           '--epoch', '1', '--save_freq', '1', '--no_train_gen', '--genc_fmaps', '8', '16', '32',
           '--denc_fmaps', '8', '16', '32', '--genc_poolings', '4', '4', '4', '--denc_poolings',
           '4', '4', '4', '--z_dim', '32', '--slice_size', '1024', '--num_workers', '0']
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert 'btime' in out.stdout and 'nan' not in out.stdout.lower()
    banks = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith('BANK')]
    assert banks[-1] == ['rir_0000.wav', 'rir_0001.wav', 'synthetic0', 'synthetic1', 'synthetic2']
    taps = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith('TAPS')]
    assert taps[-1] == ['512'] * 5
    names = [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith('NAMES')]
    assert names and all(n == 'u0_reverb' for batch in names for n in batch), names
