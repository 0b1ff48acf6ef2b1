"""The float64 numpy oracle of the reverberation augmentation: what
`ops.reverb_rows` / `augment.Reverb` compute on the MI355X, stated directly.

For one row with signal x (valid samples 0 .. len-1, an optional previous sample x[-1] = prev, zero
elsewhere) and a room impulse response h of L taps whose direct path is tap d:

    y[n] = sum_{k=0}^{L-1} h[k] x[n + d - k],   n = -1 .. len-1

y[-1] is returned apart (prev_out: what the pre-emphasis of a slice that does not start its wav
needs); y[n] = 0 for n >= len.  The slice is reverberated as if silence preceded x[-1].

The bank normalises each RIR once, in float64: cut to max_taps, d = argmax |h| (first occurrence),
h / h[d], one rounding to float32 — the direct path keeps its place and has gain exactly 1.
"""
import numpy as np


def normalise(h, max_taps=16384):
    """(float32 taps, d) of the bank's normalisation; an all-zero (or empty) RIR raises.  The
    product's copy is augment.RIRBank._normalise: keep the two alike."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)[:int(max_taps)]
    if h.size == 0 or not np.any(h != 0):
        raise ValueError('RIR without a non-zero tap (within max_taps={})'.format(max_taps))
    if not np.all(np.isfinite(h)):
        raise ValueError('RIR with a non-finite tap')
    d = int(np.argmax(np.abs(h)))
    return (h / h[d]).astype(np.float32), d


def reverb(x, h, d, length=None, prev=None):
    """(y float64 [T], prev_out float64) for the row x [T], taps h (as stored: float32 or float64
    values, used as float64) and direct-path index d."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    T = len(x)
    n = T if length is None else int(length)
    if not (0 <= n <= T and 0 <= d < len(h)):
        raise ValueError('reverb: length {} of {} / delay {} of {} taps'.format(n, T, d, len(h)))
    xe = np.concatenate(([0.0 if prev is None else float(prev)], x[:n]))    # xe[m] = x[m - 1]
    full = np.convolve(xe, h)               # full[m] = sum_k h[k] xe[m - k], len(xe) + L - 1 long
    y = np.zeros(T)
    y[:n] = full[d + 1:d + 1 + n]
    return y, float(full[d])


def scale(x, h, d, length=None, prev=None):
    """max_n (|h| * |x|)[n] over n = -1 .. len-1: what the error of a float32 evaluation is
    measured against."""
    y, p = reverb(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(h, dtype=np.float64)),
                  d, length, None if prev is None else abs(float(prev)))
    return max(float(y.max()) if len(y) else 0.0, p)
