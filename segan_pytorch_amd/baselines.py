"""Statistical-model baseline enhancers on the MI355X: the "Wiener" row of
the SEGAN paper's tables and its log-MMSE sibling, so that a checkpoint can be compared with a
classical enhancer without leaving the project.

    from segan_pytorch_amd import baselines
    y = baselines.logmmse(noisy)                 # [T] or [rows, T], fp32 or fp64 CUDA tensor
    y = baselines.wiener(noisy, lengths=lens)

Both are `ops.denoise_rows`: 20 ms Hamming frames at half overlap, the decision-directed a-priori
SNR, a noise spectrum taken from the first 120 ms and tracked through a likelihood-ratio VAD, all
in fp64 on the device.  The definition is the numpy oracle scripts/denoise_oracle.py, written from
the literature; the numbers compare systems evaluated with this tool and do not reproduce tables
made with Loizou's MATLAB programs."""
from . import ops

RULES = tuple(sorted(ops.DENOISE_RULES))


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
