"""Host side of fwSNRseg, the cepstrum distance and SI-SDR (the numpy oracle
scripts/measures_oracle.py, the fixture tests/golden/measures.pt, the header, the CLI flags, the
argument checks of ops): no GPU."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import abi_header as H
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import make_golden_measures as GM  # noqa: E402
import measures_oracle as M  # noqa: E402


@pytest.fixture(scope='module')
def qfx():
    return load_golden('quality.pt')


@pytest.fixture(scope='module')
def mfx():
    return load_golden('measures.pt')


def test_geometry_and_frame_counts():
    assert M.geometry(16000) == (480, 120, 1024, 16)
    assert M.geometry(8000) == (240, 60, 512, 10)
    assert [M.frame_count(n, 16000) for n in (1, 599, 600, 719, 720, 40000)] == [0, 0, 1, 1, 2, 329]
    assert M.crit_filters(16000).shape == (25, 512) and M.crit_filters(8000).shape == (25, 256)


@pytest.mark.parametrize('P', [10, 16])
def test_cepstrum_of_one_pole_is_the_closed_form(P):
    for a in (0.9, -0.5, 0.3):
        A = np.zeros(P + 1)
        A[0], A[1] = 1.0, -a
        want = np.array([a ** n / n for n in range(1, P + 1)])
        assert np.abs(M.cepstrum(A) - want).max() <= 1e-15


@pytest.mark.parametrize('P', [10, 16])
def test_levinson_solves_the_normal_equations(P):
    rng = np.random.default_rng(P)
    fr = rng.standard_normal(480) * M.window(480)
    R = M.lags(fr, P)
    A = M.levinson(R)
    T = np.array([[R[abs(i - j)] for j in range(P)] for i in range(P)])
    assert A[0] == 1.0 and np.abs(T @ A[1:] + R[1:]).max() <= 1e-9 * R[0]


def test_identical_signals_are_35_dB_and_zero_distance(qfx):
    for name in ('snr10', 'sr8k'):
        ref, _, sr = GM.case_signals(qfx, name)
        fw = M.fwsegsnr_frames(ref, ref, sr)
        cd = M.cd_frames(ref, ref, sr)
        assert fw.size == M.frame_count(len(ref), sr) > 0
        assert np.all(fw == 35.0) and np.all(cd == 0.0)
        assert M.fwsegsnr(ref, ref, sr) == 35.0 and M.cepstral_distance(ref, ref, sr) == 0.0


def test_silent_frames_are_nan_and_leave_the_means(qfx, mfx):
    ref, deg, sr = GM.case_signals(qfx, 'zero_run')
    fw, cd = M.fwsegsnr_frames(ref, deg, sr), M.cd_frames(ref, deg, sr)
    # frames wholly inside the zeros: f * 120 >= 20000 and f * 120 + 480 <= 22000
    inside = np.array([20000 <= f * 120 and f * 120 + 480 <= 22000 for f in range(fw.size)])
    assert inside.sum() == mfx['meta']['zero_run_nan_frames'] == 13
    assert np.array_equal(np.isnan(fw), inside) and np.array_equal(np.isnan(cd), inside)
    assert M.finite_mean(fw) == fw[~inside].mean()
    keep = np.sort(cd[~inside])[:M.trimmed_count((~inside).sum())]
    assert M.trimmed_mean(cd) == keep.mean()
    assert math.isnan(M.finite_mean(fw[inside])) and math.isnan(M.trimmed_mean(cd[inside]))
    # silence in the processed signal alone, and a signal shorter than a frame
    assert np.isnan(M.fwsegsnr_frames(deg, ref, sr)[inside]).all()
    assert np.isnan(M.cd_frames(deg, ref, sr)[inside]).all()
    assert math.isnan(M.fwsegsnr(ref[:599], deg[:599], sr))
    assert math.isnan(M.cepstral_distance(ref[:599], deg[:599], sr))


def test_si_sdr_is_invariant_to_scale_and_offset(qfx):
    ref, deg, _ = GM.case_signals(qfx, 'snr10')
    base = M.si_sdr(ref, deg)
    x = deg.astype(np.float64)
    for g, dc in ((0.25, 0.0), (-3.0, 0.0), (1.0, 0.4), (7.5, -0.2)):
        assert abs(M.si_sdr(ref, g * x + dc) - base) <= 1e-10, (g, dc)
        assert abs(M.si_sdr_moments(ref, g * x + dc) - base) <= 1e-10, (g, dc)


def test_si_sdr_of_orthogonal_noise_is_the_energy_ratio():
    rng = np.random.default_rng(3)
    n = 4001
    s = rng.standard_normal(n)
    s -= s.mean()
    noise = rng.standard_normal(n)
    basis = np.stack([s / np.linalg.norm(s), np.ones(n) / math.sqrt(n)])
    for _ in range(2):      # twice: the second pass removes the first's rounding
        noise = noise - basis.T @ (basis @ noise)
    for g in (1.0, 0.1, 1e-3):
        want = 10 * math.log10(np.dot(s, s) / np.dot(g * noise, g * noise))
        assert abs(M.si_sdr(s, s + g * noise) - want) <= 1e-9, g


def test_si_sdr_inf_and_nan():
    rng = np.random.default_rng(4)
    s = rng.standard_normal(1000).astype(np.float32)
    assert M.si_sdr(s, s) == math.inf and M.si_sdr_moments(s, s) == math.inf
    assert math.isnan(M.si_sdr(np.zeros(1000), s)) and math.isnan(M.si_sdr_moments(np.zeros(1000), s))
    assert math.isnan(M.si_sdr(s[:1], s[:1])) and math.isnan(M.si_sdr_moments(s[:1], s[:1]))


def test_recipe_reproduces_the_fixture(qfx, mfx):
    assert mfx['cases'] == GM.CASES and set(mfx['results']) == set(GM.CASES)
    for name in GM.CASES:
        ref, deg, sr = GM.case_signals(qfx, name)
        got, want = GM.evaluate(ref, deg, sr), mfx['results'][name]
        for k in ('fw_frames', 'cd_frames'):
            w = want[k].numpy()
            assert got[k].shape == w.shape == (M.frame_count(len(ref), sr),)
            assert np.array_equal(np.isnan(got[k]), np.isnan(w)), (name, k)
            assert np.nanmax(np.abs(got[k] - w)) <= 1e-11, (name, k)
        for k in ('fw', 'cd', 'sisdr'):
            assert abs(got[k] - want[k]) <= 1e-11, (name, k)
    for k, t in mfx['cli'].items():
        got = [GM.evaluate(c, n, 16000)[k] for c, n in GM.cli_signals(qfx)]
        assert np.abs(np.array(got) - t.numpy()).max() <= 1e-11, k


def test_fixture_is_small_stores_no_signals_and_bounds_the_tolerances(mfx):
    size = os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'measures.pt'))
    assert size < 64 * 1024, size
    meta = mfx['meta']
    assert 'signals' not in mfx and meta['signals'] == 'tests/golden/quality.pt'
    assert 0 < meta['cd_sensitivity_max'] and 1e-9 <= GM.cd_tolerance(meta) <= 1e-4
    assert meta['sisdr_moments_gap'] < 1e-9
    r = mfx['results']
    assert r['snr0']['fw'] < r['snr10']['fw'] < r['snr20']['fw']
    assert r['snr0']['cd'] > r['snr10']['cd'] > r['snr20']['cd']
    assert r['snr0']['sisdr'] < r['snr10']['sisdr'] < r['snr20']['sisdr']


def test_abi_entries_are_additive():
    from segan_pytorch_amd import _lib
    assert H.macro('SEGAN_ABI_VERSION') == 17 and _lib.ABI_VERSION == 17
    assert re.search(r'\bint segan_fwsegsnr\(const float\* ref, const float\* deg, const int\* '
                     r'lengths, int rows, int T,\s+int srate, double\* frames_out, double\* '
                     r'row_out, void\* stream\);', H.CODE)
    assert re.search(r'\bint segan_cepdist\(const float\* ref, const float\* deg, const int\* '
                     r'lengths,', H.CODE)
    assert re.search(r'\bint segan_sisdr\(const float\* ref, const float\* deg, const int\* '
                     r'lengths, int rows, int T,\s+double\* row_out, double\* ws, void\* '
                     r'stream\);', H.CODE)
    for name, nargs in (('segan_fwsegsnr', 9), ('segan_cepdist', 8), ('segan_sisdr', 8)):
        assert len(_lib.SIGNATURES[name][1]) == nargs
    lib = _lib.load()
    assert lib.segan_abi_version() == 17
    # arguments are checked before any launch: no device is needed to be refused
    assert lib.segan_fwsegsnr(None, None, None, 1, 4000, 16000, None, None, None) != 0
    assert b'fwsegsnr' in lib.segan_last_error()
    assert lib.segan_cepdist(None, None, None, 1, 4000, 16000, None, None) != 0
    assert b'cepdist' in lib.segan_last_error()
    assert lib.segan_sisdr(None, None, None, 1, 4000, None, None, None) != 0
    assert b'sisdr' in lib.segan_last_error()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert all(n in doc for n in ('segan_fwsegsnr', 'segan_cepdist', 'segan_sisdr'))
    from segan_pytorch_amd import ops
    assert H.macro('SEGAN_SISDR_SPAN') == ops.SISDR_SPAN


def test_eval_cli_flags_and_unchanged_header_line():
    import eval_noisy_performance as ev
    req = ['--test_wavs', 'a', '--clean_wavs', 'b', '--logfile', 'c']
    o = ev.build_parser().parse_args(req)
    assert (o.fwsegsnr, o.cd, o.sisdr, o.stoi, o.estoi) == (False,) * 5
    o = ev.build_parser().parse_args(req + ['--fwsegsnr', '--cd', '--sisdr'])
    assert (o.fwsegsnr, o.cd, o.sisdr, o.stoi, o.estoi) == (True, True, True, False, False)
    parse = lambda *flags: ev.build_parser().parse_args(req + list(flags))  # noqa: E731
    assert ev.header_line(parse()) == 'FILE CSIG CBAK COVL PESQ SSNR'
    assert ev.header_line(parse('--stoi', '--estoi')) == 'FILE CSIG CBAK COVL PESQ SSNR STOI ESTOI'
    assert ev.header_line(parse('--sisdr', '--cd', '--fwsegsnr', '--estoi')) == \
        'FILE CSIG CBAK COVL PESQ SSNR ESTOI FWSEGSNR CD SISDR'
    assert ev.header_line(parse('--cd')) == 'FILE CSIG CBAK COVL PESQ SSNR CD'


def test_train_parses_the_eval_flags():
    import train
    d = train.build_parser().parse_args([])
    assert (d.eval_fwsegsnr, d.eval_cd, d.eval_sisdr, d.eval_estoi) == (False,) * 4
    o = train.build_parser().parse_args(['--eval_fwsegsnr', '--eval_cd', '--eval_sisdr'])
    assert (o.eval_fwsegsnr, o.eval_cd, o.eval_sisdr, o.eval_stoi) == (True, True, True, False)


def test_cpu_tensors_are_refused():
    from segan_pytorch_amd import ops, quality
    x = torch.zeros(2, 4000)
    for fn in (ops.fwsegsnr, ops.cepstral_distance, ops.si_sdr, quality.fwsegsnr,
               quality.cepstral_distance, quality.si_sdr):
        with pytest.raises(RuntimeError, match='MI355X'):
            fn(x, x)


class _FakeCuda(torch.Tensor):
    """A CPU tensor that claims to be on the device: reaches the checks behind `is_cuda`."""
    is_cuda = True


def _fake(rows, T, dtype=torch.float32):
    return torch.zeros(rows, T, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize('fn', ['fwsegsnr', 'cepstral_distance', 'si_sdr'])
def test_ops_argument_checks_raise_before_any_launch(fn):
    from segan_pytorch_amd import ops
    f = getattr(ops, fn)
    x = _fake(2, 4000)
    with pytest.raises(ValueError, match='shapes differ'):
        f(x, _fake(2, 3999))
    with pytest.raises(ValueError, match='2 dims'):
        f(_fake(2, 4000)[0], _fake(2, 4000)[0])
    with pytest.raises(TypeError, match='float32'):
        f(_fake(2, 4000, torch.float64), _fake(2, 4000, torch.float64))
    for bad in ([4000], [4000, 4001], [0, 4000], [-1, 4000], [4000.0, 4000.0], [[4000, 4000]],
                [True, False]):
        with pytest.raises(ValueError, match='lengths'):
            f(x, x, lengths=bad)
    if fn != 'si_sdr':
        for bad in (0, -16000, 16000.0, True):
            with pytest.raises(ValueError, match='srate'):
                f(x, x, srate=bad)
