"""Import-compatibility alias of the reference's objective evaluation helpers (segan/utils.py):
numpy in, numpy / python values out, computed on the MI355X by segan_pytorch_amd.quality, and of
its additive-noise mixer (`Additive`, `ComposeAdditive`: segan_pytorch_amd.augment)."""
import numpy as _np
import torch as _torch

from segan_pytorch_amd import ops as _ops
from segan_pytorch_amd import quality as _q
from segan_pytorch_amd.augment import Additive, ComposeAdditive  # noqa: F401

# the evaluation names; Additive / ComposeAdditive are imported by name (`from segan.utils import
# Additive`), as the reference's train.py does
__all__ = ['CompositeEval', 'eval_composite', 'SSNR', 'wss', 'llr', 'PESQ']


def _dev(x):
    if not _torch.cuda.is_available():
        raise RuntimeError('segan_pytorch_amd runs only on an MI355X (HIP) device; there is no '
                           'CPU path')
    return _torch.as_tensor(_np.asarray(x, dtype=_np.float32).reshape(1, -1)).cuda()


def CompositeEval(ref_wav, deg_wav, log_all=False):
    """(Csig, Cbak, Covl[, pesq, segSNR]) as floats (utils.py:397-440)."""
    r = _q.composite_eval(_dev(ref_wav), _dev(deg_wav))
    keys = ('csig', 'cbak', 'covl', 'pesq', 'ssnr') if log_all else ('csig', 'cbak', 'covl')
    return tuple(float(r[k][0]) for k in keys)


def eval_composite(clean_utt, Genh_utt, noisy_utt=None):
    """utils.py:299-316: dict(s) of csig / cbak / covl / pesq / ssnr."""
    keys = ('csig', 'cbak', 'covl', 'pesq', 'ssnr')
    evals = dict(zip(keys, CompositeEval(_np.reshape(clean_utt, -1), _np.reshape(Genh_utt, -1),
                                         True)))
    if noisy_utt is None:
        return evals
    return evals, dict(zip(keys, CompositeEval(_np.reshape(clean_utt, -1),
                                               _np.reshape(noisy_utt, -1), True)))


def SSNR(ref_wav, deg_wav, srate=16000, eps=1e-10):
    """(overall SNR, list of per-frame segmental SNRs) (utils.py:350-395)."""
    snr, _, seg = _ops.ssnr(_dev(ref_wav), _dev(deg_wav), srate, eps)
    return float(snr[0]), seg[0].double().cpu().tolist()


def wss(ref_wav, deg_wav, srate):
    """List of per-frame weighted spectral slope distortions (utils.py:442-596)."""
    return _ops.wss(_dev(ref_wav), _dev(deg_wav), srate)[0].cpu().tolist()


def llr(ref_wav, deg_wav, srate):
    """ndarray of per-frame log-likelihood ratios (utils.py:598-657)."""
    return _ops.llr(_dev(ref_wav), _dev(deg_wav), srate)[0].cpu().numpy()


def PESQ(ref_wav, deg_wav):
    """pesqmain's result string (utils.py:318-347), None without pesqmain on PATH."""
    return _q.pesq_raw(ref_wav, deg_wav)
