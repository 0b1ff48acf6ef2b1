"""Host side of the speech-quality evaluation (segan_pytorch_amd/quality.py, segan/utils.py,
eval_noisy_performance.py): the fixture, the trimmed count, the pesqmain protocol."""
import os
import stat
import subprocess
import sys

import numpy as np

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_holds_what_the_gpu_tests_need():
    fx = load_golden('quality.pt')
    assert set(fx['recipes']) == {'snr0', 'snr10', 'snr20', 'white', 'zero_run', 'short',
                                  'unequal', 'sr8k'}
    for name, res in fx['results'].items():
        assert res['wss'].shape == res['llr'].shape == res['ssnr'].shape, name
        if fx['recipes'][name].get('srate', 16000) == 16000:
            assert set(res['composite']) == {'2.500', '3.100', 'error!'}
    assert fx['results']['short']['wss'].numel() == 0
    assert len(fx['cli']['names']) == len(fx['cli']['rows']) == 3
    assert fx['meta']['llr_fp32_vs_fp64_max_abs'] < 1e-4


def test_trimmed_count_reproduces_the_reference_rule():
    from segan_pytorch_amd.quality import trimmed_count
    from segan_pytorch_amd import _lib
    assert trimmed_count(30) == 28 and trimmed_count(10) == 10 and trimmed_count(0) == 0
    fx = load_golden('quality.pt')
    for name, rc in fx['recipes'].items():
        n = fx['results'][name]['wss'].numel()
        T = min(rc['len_ref'], rc['len_deg'])
        sr = rc.get('srate', 16000)
        win = round(30 * sr / 1000.)
        assert n == max(0, int(T / (win // 4) - win / (win // 4)))
        assert trimmed_count(n) == int(round(len(list(range(n))) * 0.95))


def _fake(tmp_path, body):
    exe = tmp_path / 'bin' / 'pesqmain'
    exe.parent.mkdir(exist_ok=True)
    exe.write_text('#!/bin/sh\n' + body)
    exe.chmod(exe.stat().st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(exe.parent)


def test_pesq_through_a_fake_pesqmain(tmp_path, monkeypatch):
    from scipy.io import wavfile
    from segan_pytorch_amd import quality
    log = tmp_path / 'args.txt'
    body = ('echo "$@" > {log}\ncp "$1" {d}/ref_copy.wav\ncp "$2" {d}/deg_copy.wav\n'
            'echo "P.862 Prediction (Raw MOS, MOS-LQO):  = 2.103\t2.871"\n').format(
                log=log, d=tmp_path)
    monkeypatch.setenv('PATH', _fake(tmp_path, body) + os.pathsep + os.environ['PATH'])
    x = np.array([0.0, 0.5, -1.0, 1.5, 1e-5], dtype=np.float32)
    assert quality.pesq_score(x, x * 0.5) == 2.871
    args = log.read_text().split()
    assert args[2:] == ['+16000', '+wb'] and len(args) == 4
    for a in args[:2]:
        assert not os.path.exists(a)      # temp wavs deleted
    rate, pcm = wavfile.read(str(tmp_path / 'ref_copy.wav'))
    assert rate == 16000 and pcm.dtype == np.int16
    assert pcm.tolist() == [0, 16384, -32767, 32767, 0]


def test_pesq_error_gives_minus_one(tmp_path, monkeypatch):
    from segan_pytorch_amd import quality
    monkeypatch.setenv('PATH', _fake(tmp_path, 'echo "An error! occurred"\necho\n') + os.pathsep +
                       os.environ['PATH'])
    x = np.zeros(100, dtype=np.float32)
    assert quality.pesq_score(x, x) == -1.0


def test_missing_pesqmain_gives_nan_and_one_message(tmp_path):
    code = ('import sys; sys.path.insert(0, {!r})\n'
            'import numpy as np, math\n'
            'from segan_pytorch_amd import quality\n'
            'x = np.zeros(10, dtype=np.float32)\n'
            'assert math.isnan(quality.pesq_score(x, x)) and math.isnan(quality.pesq_score(x, x))\n'
            ).format(ROOT)
    env = dict(os.environ, PATH=str(tmp_path))
    p = subprocess.run([sys.executable, '-c', code], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, env=env, universal_newlines=True, timeout=300)
    assert p.returncode == 0, p.stdout
    assert p.stdout.count('pesqmain not found! Please add it your PATH') == 1, p.stdout


def test_segan_utils_exports_the_six_names():
    import segan.utils as U
    assert sorted(U.__all__) == sorted(['CompositeEval', 'eval_composite', 'SSNR', 'wss', 'llr',
                                        'PESQ'])
    assert all(callable(getattr(U, n)) for n in U.__all__)
    assert not hasattr(U, 'make_divN')


def test_eval_cli_refuses_without_a_hip_device(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1',
               ROCR_VISIBLE_DEVICES='-1')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'eval_noisy_performance.py'),
                        '--test_wavs', str(tmp_path), '--clean_wavs', str(tmp_path),
                        '--logfile', str(tmp_path / 'log')],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env,
                       universal_newlines=True, timeout=300)
    assert p.returncode != 0
    assert 'runs only on an MI355X (HIP) device' in p.stdout
    assert not (tmp_path / 'log').exists()
