"""Host helpers around `ops.resample`: wav arrays of any rate -> 16 kHz (or
any other rate) on the MI355X.  int16 stays int16 (rounded half to even, saturated), every float
dtype becomes float32; multi-channel arrays ([samples, channels], as scipy reads them) are averaged
first, as `augment.NoiseBank` does.  One filter default for every layer: `ops.RESAMPLE_ZEROS`,
`ops.RESAMPLE_BETA` = (32, 8.6); (10, 5.0) is scipy's default."""
import numpy as np
import torch

from . import ops

TARGET_RATE = 16000
MAX_BATCH_SAMPLES = 1 << 24      # padded input samples per device call of resample_many


def add_filter_flags(parser):
    """--resample_zeros / --resample_beta of every command line that converts rates."""
    parser.add_argument('--resample_zeros', type=int, default=ops.RESAMPLE_ZEROS,
                        help='zero crossings a side of the conversion filter (1 .. 64; 10 with '
                             '--resample_beta 5.0 is scipy\'s default)')
    parser.add_argument('--resample_beta', type=float, default=ops.RESAMPLE_BETA,
                        help='Kaiser beta of the conversion filter (0 .. 20)')


def _device(device):
    if not torch.cuda.is_available():
        raise RuntimeError('resample: segan_pytorch_amd runs only on an MI355X (HIP) device; there is '
                           'no CPU path')
    return torch.device('cuda' if device is None else device)


def as_mono(array):
    """numpy int16 [n] kept; int16 [n, ch] and every float array -> float32 (channels averaged)."""
    a = np.asarray(array)
    if a.dtype != np.int16 and not np.issubdtype(a.dtype, np.floating):
        raise TypeError('resample: wav arrays must be int16 or float, got {}'.format(a.dtype))
    if a.ndim == 2:
        a = a.mean(axis=1, dtype=np.float32 if a.dtype == np.int16 else None)
    elif a.ndim != 1:
        raise ValueError('resample: wav arrays are [samples] or [samples, channels], got shape '
                         '{}'.format(a.shape))
    if a.dtype != np.int16:
        a = a.astype(np.float32)
    return np.ascontiguousarray(a)


def resample_many(arrays, rates, rate_out=TARGET_RATE, zeros=ops.RESAMPLE_ZEROS,
                  beta=ops.RESAMPLE_BETA, device=None, max_batch_samples=MAX_BATCH_SAMPLES):
    """Convert wav arrays of the given rates (one int per array, or one int for all) to `rate_out`.
    Arrays already at rate_out come back as they are (the same objects).  The others are grouped
    by (rate, int16-ness), padded to their group's longest and converted in device calls of at
    most `max_batch_samples` padded input samples (a single longer array goes alone).  Returns
    (list of arrays in the input's order, saturated samples in total)."""
    arrays = list(arrays)
    rates = [int(rates)] * len(arrays) if np.isscalar(rates) else [int(r) for r in rates]
    if len(rates) != len(arrays):
        raise ValueError('resample_many: {} rates for {} arrays'.format(len(rates), len(arrays)))
    out = list(arrays)
    groups = {}
    for i, (a, r) in enumerate(zip(arrays, rates)):
        if r == rate_out:
            continue
        out[i] = as_mono(a)
        if len(out[i]) == 0:
            raise ValueError('resample_many: array {} is empty'.format(i))
        groups.setdefault((r, out[i].dtype == np.int16), []).append(i)
    dev = _device(device) if groups else None
    nclip = 0
    for (rate, is_i16), idx in sorted(groups.items()):
        idx.sort(key=lambda i: len(out[i]))      # similar lengths share a call: less padding
        beg = 0
        while beg < len(idx):
            end = beg + 1
            while end < len(idx) and end - beg < 65535 and \
                    (end - beg + 1) * len(out[idx[end]]) <= max_batch_samples:
                end += 1
            part = idx[beg:end]
            T = len(out[part[-1]])
            host = np.zeros((len(part), T), dtype=np.int16 if is_i16 else np.float32)
            for k, i in enumerate(part):
                host[k, :len(out[i])] = out[i]
            lens = [len(out[i]) for i in part]
            y, info = ops.resample(torch.from_numpy(host).to(dev), rate, rate_out, lengths=lens,
                                   zeros=zeros, beta=beta)
            y = y.cpu().numpy()
            got = info['lengths'].cpu().tolist()
            nclip += int(info['nclip'].sum().item())
            for k, i in enumerate(part):
                out[i] = y[k, :got[k]].copy()
            beg = end
    return out, nclip


def resample_wav(array, rate_in, rate_out=TARGET_RATE, zeros=ops.RESAMPLE_ZEROS,
                 beta=ops.RESAMPLE_BETA, device=None):
    """One wav array at rate_in -> rate_out on the GPU: int16 -> int16, float -> float32
    ([samples, channels] averaged first).  At rate_in == rate_out the array is returned as it is."""
    return resample_many([array], [rate_in], rate_out, zeros, beta, device)[0][0]
