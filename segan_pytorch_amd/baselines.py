"""Classical baselines on the MI355X: the statistical-model enhancers, the
"Wiener" row of the SEGAN paper's tables and its log-MMSE sibling, and the WPE dereverberator
(section 21), so that a checkpoint can be compared with a classical enhancer without leaving the
project.

    from segan_pytorch_amd import baselines
    y = baselines.logmmse(noisy)                 # [T] or [rows, T], fp32 or fp64 CUDA tensor
    y = baselines.wiener(noisy, lengths=lens)
    y = baselines.wpe(reverberant)               # `wpe` and `wpe_wav`: see their own docstrings

The two enhancers are `ops.denoise_rows`: 20 ms Hamming frames at half overlap, the
decision-directed a-priori SNR, a noise spectrum taken from the first 120 ms and tracked through a likelihood-ratio VAD, all
in fp64 on the device.  The definition is the numpy oracle scripts/denoise_oracle.py, written from
the literature; the numbers compare systems evaluated with this tool and do not reproduce tables
made with Loizou's MATLAB programs."""
from . import ops

RULES = tuple(sorted(ops.DENOISE_RULES))
WPE_DEFAULTS = {'taps': 10, 'delay': 3, 'iterations': 3}


def denoise(x, srate=16000, lengths=None, rule='logmmse'):
    """Each row of x enhanced with `rule` ('wiener' or 'logmmse') at `srate` (16000 or 8000); the
    result has x's shape and dtype.  `lengths`: host integers, row r is x[r, :lengths[r]]."""
    return ops.denoise_rows(x, lengths=lengths, srate=srate, rule=rule)


def wiener(x, srate=16000, lengths=None):
    """The a-priori-SNR Wiener filter G = xi / (1 + xi) of Scalart & Filho (1996)."""
    return denoise(x, srate, lengths, 'wiener')


def logmmse(x, srate=16000, lengths=None):
    """The log-spectral-amplitude MMSE estimator of Ephraim & Malah (1985)."""
    return denoise(x, srate, lengths, 'logmmse')


def denoise_wav(wav, rule='logmmse', srate=16000, device='cuda'):
    """A wav array as scipy reads it ([samples], int16 or float) enhanced on the device: int16 is
    scaled by 1 / 32768, enhanced, scaled back, rounded to nearest (half to even) and clipped to
    int16; a float array comes back as float32."""
    import numpy as np
    import torch
    a = np.asarray(wav)
    if a.ndim != 1 or not (a.dtype == np.int16 or np.issubdtype(a.dtype, np.floating)):
        raise TypeError('denoise_wav: a one-dimensional int16 or float array, got {} {}'.format(
            a.dtype, a.shape))
    if a.dtype == np.int16:
        x = torch.from_numpy(a.astype(np.float32) / 32768).to(device)
        y = ops.denoise_rows(x, srate=srate, rule=rule, out_dtype=torch.float64)
        return np.clip(np.rint(y.cpu().numpy() * 32768.0), -32768, 32767).astype(np.int16)
    x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return ops.denoise_rows(x, srate=srate, rule=rule).cpu().numpy()


def wpe(x, srate=16000, lengths=None, taps=10, delay=3, iterations=3):
    """The WPE dereverberation of each row of x (weighted prediction error, Nakatani et al. 2010,
    single channel) at `srate` (16000 or 8000): `ops.wpe_rows`, whose
    definition is the numpy oracle scripts/wpe_oracle.py, written from the literature.  The result
    has x's shape and dtype.  `lengths`: host integers, row r is x[r, :lengths[r]].  WPE assumes
    that the source is uncorrelated beyond `delay` frames: a steady tone is predictable from its
    own past and is cancelled with its reverberation."""
    return ops.wpe_rows(x, lengths=lengths, srate=srate, taps=taps, delay=delay,
                        iterations=iterations)


def wpe_wav(wav, srate=16000, taps=10, delay=3, iterations=3, device='cuda'):
    """A wav array as scipy reads it ([samples], int16 or float) dereverberated on the device, as
    `denoise_wav` enhances one: int16 is scaled by 1 / 32768, processed, scaled back, rounded to
    nearest (half to even) and clipped to int16; a float array comes back as float32."""
    import numpy as np
    import torch
    a = np.asarray(wav)
    if a.ndim != 1 or not (a.dtype == np.int16 or np.issubdtype(a.dtype, np.floating)):
        raise TypeError('wpe_wav: a one-dimensional int16 or float array, got {} {}'.format(
            a.dtype, a.shape))
    kw = dict(srate=srate, taps=taps, delay=delay, iterations=iterations)
    if a.dtype == np.int16:
        x = torch.from_numpy(a.astype(np.float32) / 32768).to(device)
        y = ops.wpe_rows(x, out_dtype=torch.float64, **kw)
        return np.clip(np.rint(y.cpu().numpy() * 32768.0), -32768, 32767).astype(np.int16)
    x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return ops.wpe_rows(x, **kw).cpu().numpy()


def add_wpe_flags(parser):
    """--wpe, --wpe_taps, --wpe_delay, --wpe_iterations of clean.py and eval_noisy_performance.py:
    absent from the namespace unless given, so the default namespaces stay as they were."""
    import argparse
    parser.add_argument('--wpe', action='store_true', default=argparse.SUPPRESS,
                        help='dereverberate every file with WPE first (before --baseline RULE if '
                             'that is given too); needs neither --cfg_file nor a checkpoint')
    for key, lo_hi in (('taps', '1 .. 32'), ('delay', 'in frames, 1 .. 8'),
                       ('iterations', '0 .. 8')):
        parser.add_argument('--wpe_' + key, type=int, default=argparse.SUPPRESS,
                            help='prediction {} of --wpe, {} (default {})'.format(
                                key, lo_hi, WPE_DEFAULTS[key]))


def wpe_opts(opts):
    """None without --wpe, else the keyword arguments of `wpe` / `wpe_wav` of a parsed namespace."""
    if not getattr(opts, 'wpe', False):
        for k in WPE_DEFAULTS:
            if hasattr(opts, 'wpe_' + k):
                raise SystemExit('--wpe_{} needs --wpe'.format(k))
        return None
    return {k: getattr(opts, 'wpe_' + k, v) for k, v in WPE_DEFAULTS.items()}
