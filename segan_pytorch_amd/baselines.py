"""Classical baselines on the MI355X: the statistical-model enhancers, the
"Wiener" row of the SEGAN paper's tables and its log-MMSE sibling, the WPE dereverberator
(section 21) and the OM-LSA enhancer with IMCRA noise tracking (section 23), so that a checkpoint
can be compared with a classical enhancer without leaving the project.

    from segan_pytorch_amd import baselines
    y = baselines.logmmse(noisy)                 # [T] or [rows, T], fp32 or fp64 CUDA tensor
    y = baselines.wiener(noisy, lengths=lens)
    y = baselines.wpe(reverberant)               # `wpe` and `wpe_wav`: see their own docstrings
    y = baselines.omlsa(noisy)                   # `omlsa` and `omlsa_wav`: the same

The two enhancers are `ops.denoise_rows`: 20 ms Hamming frames at half overlap, the
decision-directed a-priori SNR, a noise spectrum taken from the first 120 ms and tracked through a likelihood-ratio VAD, all
in fp64 on the device.  The definition is the numpy oracle scripts/denoise_oracle.py, written from
the literature; the numbers compare systems evaluated with this tool and do not reproduce tables
made with Loizou's MATLAB programs.  `omlsa` is `ops.omlsa_rows`: the same frames, the
log-spectral-amplitude gain weighted with the speech-presence probability, and a noise spectrum
that follows the minima of the smoothed periodogram, so it needs no leading noise segment and keeps
adapting when the noise level changes; scripts/omlsa_oracle.py is its definition, and the same
disclaimer holds for its numbers."""
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


def _wav(what, wav, device, rows, **kw):
    """`rows` (one of ops.*_rows, with `kw`) on a wav array as scipy reads it ([samples], int16 or
    float): int16 is scaled by 1 / 32768, processed with an fp64 output, scaled back, rounded to
    nearest (half to even) and clipped to int16; a float array comes back as float32."""
    import numpy as np
    import torch
    a = np.asarray(wav)
    if a.ndim != 1 or not (a.dtype == np.int16 or np.issubdtype(a.dtype, np.floating)):
        raise TypeError('{}: a one-dimensional int16 or float array, got {} {}'.format(
            what, a.dtype, a.shape))
    if a.dtype == np.int16:
        x = torch.from_numpy(a.astype(np.float32) / 32768).to(device)
        y = rows(x, out_dtype=torch.float64, **kw)
        return np.clip(np.rint(y.cpu().numpy() * 32768.0), -32768, 32767).astype(np.int16)
    x = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return rows(x, **kw).cpu().numpy()


def denoise_wav(wav, rule='logmmse', srate=16000, device='cuda'):
    """A wav array as scipy reads it ([samples], int16 or float) enhanced on the device: int16 is
    scaled by 1 / 32768, enhanced, scaled back, rounded to nearest (half to even) and clipped to
    int16; a float array comes back as float32."""
    return _wav('denoise_wav', wav, device, ops.denoise_rows, srate=srate, rule=rule)


def omlsa(x, srate=16000, lengths=None):
    """The OM-LSA enhancement of each row of x (Cohen & Berdugo 2001, with the IMCRA noise spectrum
    of Cohen 2003) at `srate` (16000 or 8000): `ops.omlsa_rows`, whose
    definition is the numpy oracle scripts/omlsa_oracle.py, written from the two papers.  The
    result has x's shape and dtype.  `lengths`: host integers, row r is x[r, :lengths[r]].  It
    takes no noise segment from the start of the row and follows a noise level that changes."""
    return ops.omlsa_rows(x, lengths=lengths, srate=srate)


def omlsa_wav(wav, srate=16000, device='cuda'):
    """A wav array as scipy reads it ([samples], int16 or float) enhanced with OM-LSA on the
    device, as `denoise_wav` enhances one: int16 is scaled by 1 / 32768, enhanced, scaled back,
    rounded to nearest (half to even) and clipped to int16; a float array comes back as float32."""
    return _wav('omlsa_wav', wav, device, ops.omlsa_rows, srate=srate)


def add_omlsa_flags(parser):
    """--omlsa of clean.py and eval_noisy_performance.py: absent from the namespace unless given,
    so the default namespaces stay as they were."""
    import argparse
    parser.add_argument('--omlsa', action='store_true', default=argparse.SUPPRESS,
                        help='enhance every file with OM-LSA on an IMCRA noise estimate (after '
                             '--wpe if that is given too; not with --baseline); needs neither '
                             '--cfg_file nor a checkpoint')


def omlsa_opts(opts):
    """Whether a parsed namespace asks for --omlsa; with --baseline RULE as well it is refused:
    one enhancer a run."""
    on = bool(getattr(opts, 'omlsa', False))
    if on and getattr(opts, 'baseline', None) is not None:
        raise SystemExit('--omlsa does not go with --baseline: each is an enhancer of its own')
    return on


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
    return _wav('wpe_wav', wav, device, ops.wpe_rows, srate=srate, taps=taps, delay=delay,
                iterations=iterations)


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
