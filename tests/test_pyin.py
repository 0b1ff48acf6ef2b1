"""The Viterbi-smoothed pitch tracker without a device: the oracle
scripts/pyin_oracle.py against slower, literal forms of itself, the library's tables against the
oracle's, the fixture tests/golden/pyin.pt against its recipe, the refusals that need no GPU, and
the comparison with YIN on the noisy gated signal of tests/golden/pitch.pt that the tracker is for.

The device parity is tests/test_gpu_pyin.py."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_pitch as GPITCH  # noqa: E402
import make_golden_pyin as GP  # noqa: E402
import pitch_oracle as P  # noqa: E402
import pyin_oracle as Y  # noqa: E402


@pytest.fixture(scope='module')
def yfx():
    return load_golden('pyin.pt')


def _tiny_A(W, dyadic):
    A = np.zeros((2, 2 * W + 1))
    for s in range(2):
        for k in range(-W, W + 1):
            A[s, k + W] = ((0.25 if s else 0.5) if dyadic else (0.01 if s else 0.99)) * (
                W + 1 - abs(k)) / (W + 1) ** 2
    return A


@pytest.mark.parametrize('F', [1, 2, 3, 5])
def test_viterbi_is_the_exhaustive_search_on_tiny_models(F):
    M, W = 3, 1
    rng = np.random.default_rng(100 + F)
    for trial in range(6):
        # random observations: the best path is unique, and its value is the decoder's own product
        B = rng.uniform(0.05, 1.0, (F, 2 * M))
        B[:, :M] *= rng.random((F, M)) < 0.7          # bins without a candidate
        A = _tiny_A(W, False)
        path, delta, gap = Y.viterbi(B, A, W)
        want, value = Y.viterbi_exhaustive(B, A, W)
        assert np.array_equal(path, want), (trial, path, want)
        assert value > 0 and gap > 0
        m, e = np.frexp(value)
        assert delta.max() == m and delta[path[-1]] == m      # the scaling is a power of two
        # tie-laden observations with dyadic weights: every product is exact, so paths of equal
        # probability tie exactly, and the lowest index wins from the last frame backwards
        B = rng.choice([0.0, 0.25, 0.5, 1.0], (F, 2 * M))
        B[:, M:] = rng.choice([0.25, 0.5], (F, 1))
        A = _tiny_A(W, True)
        path, delta, gap = Y.viterbi(B, A, W)
        want, value = Y.viterbi_exhaustive(B, A, W)
        assert np.array_equal(path, want), (trial, path, want)
        assert gap > 0                                          # exact ties are not decisions


def test_viterbi_respects_the_band():
    # the only voiced mass moves by W + 1 bins: the path cannot follow it in one step
    M, W = 6, 2
    B = np.full((2, 2 * M), 1e-3)
    B[:, :M] = 0
    B[0, 0] = B[1, W + 1] = 1.0
    path, _, _ = Y.viterbi(B, _tiny_A(W, False), W)
    assert abs(int(path[1]) % M - int(path[0]) % M) <= W
    B[1, :M] = 0
    B[1, W] = 1.0
    path, _, _ = Y.viterbi(B, _tiny_A(W, False), W)
    assert path.tolist() == [0, W]


def test_threshold_ranges_equal_the_literal_loop_over_the_thresholds(yfx):
    theta = Y.thresholds()
    frames = []
    for name, srate in (('gated5', 16000), ('tone8', 8000)):
        dp, _, ct = P.cmnd(yfx['signals'][name].numpy(), srate)
        frames += [(dp[t], srate) for t in range(0, len(dp), 3) if ct[t] > 0]
    rng = np.random.default_rng(7)
    for i in range(40):         # values on the thresholds themselves, ties, plateaus
        d = np.round(rng.uniform(0, 1.4 if i % 2 else 0.4, 268), 2)
        frames.append((d, 16000))
    frames.append((np.ones(268), 16000))
    frames.append((np.linspace(1.2, 0.0, 268), 16000))
    frames.append((np.linspace(0.0, 1.2, 268), 16000))
    seen = set()
    for d, srate in frames:
        rg, n0, star = Y.ranges(d, srate, theta)
        assert (rg, n0, star) == Y.ranges_by_stops(d, srate, theta)
        picked, none, lowest = Y.ranges_literal(d, srate, theta)
        assert none == list(range(1, n0 + 1)) and star == lowest
        assert set(picked) == set(rg)
        for tau, idx in picked.items():
            assert idx == list(range(rg[tau][0] + 1, rg[tau][1] + 1)), tau
        assert n0 + sum(hi - lo for lo, hi in rg.values()) == Y.NTHETA
        seen.add(len(rg))
    assert max(seen) >= 3 and 0 in seen


def test_tables_have_their_properties_and_the_library_has_the_oracles():
    from segan_pytorch_amd import ops
    for srate in (16000, 8000):
        t = Y.tables(srate)
        C, edge, A = t['C'], t['edge'], t['A']
        assert C.shape == (101,) and edge.shape == (166,) and A.shape == (2, 23)
        # the weights of the high thresholds fall below the rounding of a sum near 1
        assert C[0] == 0 and (np.diff(C) >= 0).all() and (np.diff(C[:60]) > 0).all()
        assert C[100] == C[99]
        assert abs(C[100] - 1) < 1e-14
        mean = float(np.sum(Y.thresholds()[1:] * np.diff(C)))
        assert abs(mean - 0.1) < 1e-3                          # Beta(2, 18)
        assert (np.diff(edge) < 0).all() and edge[0] == srate / 60.0
        assert abs(srate / edge[165] - 60 * 2 ** (33 / 12)) < 1e-9
        assert abs(edge[60] - srate / 120.0) < 1e-9            # 60 bins to the octave
        assert np.array_equal(A, A[:, ::-1]) and (A > 0).all()
        assert abs(A[0].sum() - 0.99) < 1e-15 and abs(A[1].sum() - 0.01) < 1e-16
        assert A[0, 11] == 0.99 * 12 / 144 and A[1, 0] == 0.01 * 1 / 144
        lib = ops.pyin_tables(srate)
        for k in ('C', 'edge', 'A'):
            assert lib[k].shape == t[k].shape and lib[k].dtype == np.float64
            ulp = np.spacing(np.abs(t[k]))
            assert (np.abs(lib[k] - t[k]) <= 4 * ulp).all(), k
    assert Y.bin_of(16000 / 60.0, Y.tables(16000)['edge']) == 0
    assert Y.bin_of(300.0, Y.tables(16000)['edge']) == 0       # below 60 Hz: clamped
    assert Y.bin_of(39.5, Y.tables(16000)['edge']) == 164      # above the top edge: clamped
    assert Y.bin_of(16000 / 120.5, Y.tables(16000)['edge']) == 60


def test_fixture_is_what_its_recipe_and_the_oracle_give(yfx):
    sig = GP.make_signals(yfx['meta']['seed'])
    assert set(sig) == set(yfx['signals'])
    for k, v in sig.items():
        assert np.array_equal(v, yfx['signals'][k].numpy()), k
    rows = GP.rows(sig)
    assert list(rows) == list(yfx['rows'])
    assert [len(rows['tone[:{}]'.format(L)][0]) for L in GP.PREFIXES] == [666, 667, 747, 1707, 8000]
    frames = {}
    for name, (x, srate) in rows.items():
        want = yfx['rows'][name]
        got = Y.track(x, srate)
        frames[name] = len(got['lag'])
        assert len(got['lag']) == P.n_frames(len(x), srate) and want['srate'] == srate
        for k in ('lag', 'state'):
            assert np.array_equal(got[k], want[k].numpy()), (name, k)
        for k in ('f0', 'vprob', 'delta'):
            assert np.array_equal(got[k], want[k].numpy(), equal_nan=True), (name, k)
        assert got['gap'] == want['gap'] and want['gap'] > 1e-9
        assert np.array_equal(got['lag'] > 0, got['state'] < Y.BINS)
        assert all(0 <= want['move'][k] < 1e-11 for k in ('f0', 'vprob', 'bv', 'delta'))
    assert [frames['tone[:{}]'.format(L)] for L in GP.PREFIXES] == [0, 1, 2, 14, 92]
    assert not yfx['rows']['zero']['lag'].any() and not yfx['rows']['zero']['vprob'].any()
    lead = yfx['rows']['lead']
    assert not lead['lag'][:30].any() and lead['lag'][40:].all()
    # a power of two changes no bit
    for k in ('f0', 'vprob', 'delta'):
        assert torch.equal(yfx['rows']['tone*2^-10'][k], yfx['rows']['tone[:8000]'][k])
    g = yfx['rows']['gated5']
    assert 0 < int((g['lag'] > 0).sum()) < len(g['lag'])
    o = yfx['rows']['octave']['f0'].numpy()
    assert o[:5].max() < 105 and o[-5:].min() > 195             # the glide is followed


def test_pyin_holds_where_yin_gives_way(yfx):
    """The gated harmonic signal of tests/golden/pitch.pt in white noise, each tracker against its
    own contour of the clean signal.  At 5 dB pYIN is strictly better on both counts.  At 20 dB it
    may be worse by no more than was measured when the tracker was written:
    0.0517 Hz of F0 error and one frame of 197 in voicing accuracy."""
    pfx = load_golden('pitch.pt')
    sig = {k: v.numpy() for k, v in pfx['signals'].items()}
    deg = GPITCH.processed(sig, pfx['gains'])
    cy, cp = P.track(sig['speech']), Y.track(sig['speech'])
    res = {}
    for name in ('snr20', 'snr10', 'snr5'):
        dy, dp = P.track(deg[name]), Y.track(deg[name])
        ey = P.f0_eval(cy['f0'], cy['lag'], dy['f0'], dy['lag'])
        ep = P.f0_eval(cp['f0'], cp['lag'], dp['f0'], dp['lag'])
        res[name] = (float(ey['f0_mae']), float(ey['vuv_acc']), float(ep['f0_mae']),
                     float(ep['vuv_acc']))
        print('{}: YIN f0_mae {:.4f} vuv_acc {:.4f}; pYIN f0_mae {:.4f} vuv_acc {:.4f}'.format(
            name, *res[name]))
    y_mae, y_acc, p_mae, p_acc = res['snr5']
    assert p_mae < y_mae and p_acc > y_acc
    y_mae, y_acc, p_mae, p_acc = res['snr20']
    assert p_mae - y_mae <= 0.0517 and y_acc - p_acc <= 1 / 197 + 1e-12


def test_binding_has_the_new_exports_beside_the_old_ones():
    from segan_pytorch_amd import _lib
    assert len(_lib.SIGNATURES) == 119 and _lib.ABI_VERSION == 17
    assert list(_lib.EXT_SIGNATURES) == ['segan_wpe_dims', 'segan_wpe']
    assert list(_lib.PYIN_SIGNATURES) == ['segan_pyin_tables', 'segan_pyin_dims', 'segan_pyin']
    assert [len(_lib.PYIN_SIGNATURES[n][1]) for n in _lib.PYIN_SIGNATURES] == [4, 4, 13]
    assert dict(_lib.PYIN_DEFINES) == {'SEGAN_PYIN_NTHETA': 100, 'SEGAN_PYIN_BINS': 165,
                                       'SEGAN_PYIN_W': 11}
    assert not set(_lib.PYIN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EXT_SIGNATURES))
    with pytest.raises(RuntimeError, match='not found'):
        _lib._read_header_file(_lib.PYIN_HEADER_PATH + '.missing')
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    assert lib.segan_pyin.argtypes == _lib.PYIN_SIGNATURES['segan_pyin'][1]
    assert lib.segan_pyin_dims.restype is ctypes.c_int
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        assert 'segan_pyin.h' in f.read()


def test_refusals_that_need_no_device():
    import eval_noisy_performance as ev
    import train
    from segan_pytorch_amd import _lib, ops, quality
    lib = _lib.load()
    x = torch.zeros(2, 4000)
    for fn in (ops.pyin, ops.pyin_stages):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x)
    with pytest.raises(ValueError, match='srate'):
        ops.pyin_tables(44100)
    with pytest.raises(ValueError, match='srate'):
        ops.pyin_tables(True)
    for bad in ((0, 4000, 16000), (65536, 4000, 16000), (1, 0, 16000), (1, (1 << 24) + 1, 16000),
                (1, 4000, 11025)):
        with pytest.raises(RuntimeError, match='pyin: bad sizes'):
            ops.pyin_dims(*bad)
    d = ops.pyin_dims(3, 8000, 16000)
    assert d['frames'] == 92 and d['ws_doubles'] > 3 * 92 * (268 + 2 * 165)
    assert ops.pyin_dims(1, 666)['frames'] == 0
    assert ops.pyin_dims(1, 4000, 8000)['frames'] == P.n_frames(4000, 8000)
    # the C entry points refuse before any launch
    one = ctypes.c_double()
    p = ctypes.addressof(one)
    assert lib.segan_pyin(None, None, 1, 4000, 16000, p, p, p, None, None, None, p, None) != 0
    assert b'pyin: NULL pointer' in lib.segan_last_error()
    assert lib.segan_pyin(p, None, 0, 4000, 16000, p, p, p, None, None, None, p, None) != 0
    assert b'pyin: bad sizes' in lib.segan_last_error()
    assert lib.segan_pyin(p, None, 1, 4000, 22050, p, p, p, None, None, None, p, None) != 0
    assert b'pyin: bad sizes' in lib.segan_last_error()
    assert lib.segan_pyin_tables(16000, None, p, p) != 0
    assert lib.segan_pyin_dims(1, 4000, 16000, None) != 0
    for fn in (quality.pitch, lambda a, **k: quality.f0_eval(a, a, **k)):
        with pytest.raises(ValueError, match='tracker'):
            fn(x, tracker='swipe')
        with pytest.raises(ValueError, match='tracker'):
            fn(x, tracker=None)
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x, tracker='pyin')
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    assert ev.build_parser().parse_args(req).f0_tracker == 'yin'
    o = ev.build_parser().parse_args(req + ['--f0', '--f0_tracker', 'pyin'])
    assert o.f0_tracker == 'pyin'
    assert ev.header_line(o) == ev.header_line(ev.build_parser().parse_args(req + ['--f0']))
    with pytest.raises(SystemExit):
        ev.build_parser().parse_args(req + ['--f0_tracker', 'swipe'])
    assert train.build_parser().parse_args([]).eval_f0_tracker == 'yin'
    assert train.build_parser().parse_args(['--eval_f0_tracker', 'pyin']).eval_f0_tracker == 'pyin'
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(['--eval_f0_tracker', 'swipe'])
