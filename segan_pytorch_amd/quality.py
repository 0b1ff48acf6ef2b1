"""Objective speech-quality evaluation of the reference's segan/utils.py:299-440 on the device:
CSIG / CBAK / COVL (Hu & Loizou's composite measures) from WSS, LLR, segmental SNR and PESQ, and
STOI (Taal et al.'s short-time objective intelligibility, the reference's utils/stoi.m).

The per-frame measures are HIP kernels (``ops.wss``, ``ops.llr``, ``ops.ssnr``); the trimmed means
and the three linear formulas are a few hundred numbers per row and run as torch ops on the device.
PESQ is the external ITU-T P.862 ``pesqmain`` binary, called like the reference does.
"""
import math
import os
import re
import shutil
import subprocess
import tempfile
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops

ALPHA = 0.95
SRATE = 16000
MAX_WORKERS = 16
PESQ_NOT_FOUND = 'pesqmain not found! Please add it your PATH'

_warned = False
_warn_lock = threading.Lock()


def trimmed_count(n, alpha=ALPHA):
    """How many of the n ascending frame values the alpha-trimmed mean keeps: Python's round
    (half to even) of the float product, as utils.py:410-417 (n = 30 keeps 28)."""
    return int(round(n * alpha))


def _pesq_missing():
    global _warned
    with _warn_lock:
        if not _warned:
            _warned = True
            print(PESQ_NOT_FOUND)


def pesq_raw(ref, deg, srate=SRATE):
    """The last token of ``pesqmain ref.wav deg.wav +16000 +wb``'s second-last output line (the
    string utils.py:318-347 returns), or None when pesqmain is not on PATH (the message is
    printed once per process).  Both signals go through 16-bit PCM wav files (x * 32767, rounded to
    nearest, clipped), which are deleted afterwards."""
    from scipy.io import wavfile
    exe = shutil.which('pesqmain')
    if exe is None:
        _pesq_missing()
        return None
    paths = []
    try:
        for tag, x in (('ref', ref), ('deg', deg)):
            fd, path = tempfile.mkstemp(suffix='_{}.wav'.format(tag))
            os.close(fd)
            paths.append(path)
            x = np.asarray(x, dtype=np.float64).reshape(-1)
            pcm = np.clip(np.rint(x * 32767), -32768, 32767).astype(np.int16)
            wavfile.write(path, srate, pcm)
        p = subprocess.run([exe, paths[0], paths[1], '+{}'.format(srate), '+wb'],
                           stdout=subprocess.PIPE, encoding='ascii', errors='replace')
        if 'error!' in p.stdout:
            return 'error!'
        lines = p.stdout.split('\n')
        if len(lines) < 2:
            raise RuntimeError('pesqmain: unexpected output {!r}'.format(p.stdout))
        return re.split(r'\s+', lines[-2])[-1]
    finally:
        for path in paths:
            try:
                os.remove(path)
            except OSError:
                pass


def _pesq_value(raw):
    """utils.py:421-424: a string containing 'error!' is -1, otherwise its float; None (no
    pesqmain) is NaN."""
    if raw is None:
        return math.nan
    if isinstance(raw, str):
        return -1.0 if 'error!' in raw else float(raw)
    return float(raw)


def pesq_score(ref_np, deg_np):
    """PESQ (wide band, 16 kHz) of two numpy signals through pesqmain: float, -1 on a pesqmain
    error, NaN without pesqmain."""
    return _pesq_value(pesq_raw(ref_np, deg_np))


def _trimmed_mean(frames, k):
    return torch.sort(frames, dim=1).values[:, :k].mean(dim=1)


def _as_rows(x, name):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError('{} must be a CUDA (HIP) tensor: segan_pytorch_amd runs only on an '
                           'MI355X (HIP) device; there is no CPU path'.format(name))
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2:
        raise ValueError('{} must be [rows, T] or [T], got {}'.format(name, tuple(x.shape)))
    return x


def composite_eval(ref, deg, pesq=None, workers=2):
    """CompositeEval (utils.py:397-440) of each row of ref / deg ([rows, T] or [T] CUDA tensors,
    16 kHz), truncated to the common length.  Returns a dict of fp64 device tensors [rows]:
    csig, cbak, covl, pesq, ssnr (mean segmental SNR), wss, llr (0.95-trimmed means).

    pesq: None runs pesqmain on each row (in a pool of ``min(workers, 16)`` threads); otherwise
    one value or one per row, each a number or a pesqmain result string ('error!' -> -1).

    Edge cases:
      * a row with any non-finite frame LLR (a clean frame of digital silence) has llr = NaN, and
        so csig and covl are NaN; cbak stays finite.  (The reference's result there depends on
        where Python's sort leaves the NaN.)
      * fewer samples than one frame (T < win + hop, 600 at 16 kHz): every measure is NaN, pesq
        included (pesqmain is not called).
      * without pesqmain on PATH (and pesq=None): pesq, csig, cbak and covl are NaN; wss, llr and
        ssnr are still computed.
    """
    ref = _as_rows(ref, 'ref')
    deg = _as_rows(deg, 'deg')
    if ref.shape[0] != deg.shape[0]:
        raise ValueError('ref and deg have {} and {} rows'.format(ref.shape[0], deg.shape[0]))
    L = min(ref.shape[1], deg.shape[1])
    ref = ref[:, :L].float().contiguous()
    deg = deg[:, :L].float().contiguous()
    rows, dev = ref.shape[0], ref.device
    f64 = dict(device=dev, dtype=torch.float64)

    wss_f = ops.wss(ref, deg, SRATE)
    llr_f = ops.llr(ref, deg, SRATE)
    _, _, seg = ops.ssnr(ref, deg, SRATE)
    nf = wss_f.shape[1]
    if nf == 0:
        nan = torch.full((rows,), math.nan, **f64)
        return {k: nan.clone() for k in ('csig', 'cbak', 'covl', 'pesq', 'ssnr', 'wss', 'llr')}
    k = trimmed_count(nf)
    wss_m = _trimmed_mean(wss_f, k)
    llr_m = _trimmed_mean(llr_f, k)
    llr_m = torch.where(torch.isfinite(llr_f).all(dim=1), llr_m, torch.full_like(llr_m, math.nan))
    ssnr_m = seg.double().mean(dim=1)

    if pesq is None:
        r_np, d_np = ref.cpu().numpy(), deg.cpu().numpy()
        if shutil.which('pesqmain') is None:
            _pesq_missing()
            vals = [math.nan] * rows
        elif rows == 1:
            vals = [pesq_score(r_np[0], d_np[0])]
        else:
            with ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS))) as pool:
                vals = list(pool.map(pesq_score, r_np, d_np))
    elif isinstance(pesq, (str, bytes, int, float)):
        vals = [_pesq_value(pesq)] * rows
    else:
        vals = [_pesq_value(v) for v in pesq]
        if len(vals) != rows:
            raise ValueError('pesq has {} values for {} rows'.format(len(vals), rows))
    pesq_t = torch.tensor(vals, **f64)

    csig = (3.093 - 1.029 * llr_m + 0.603 * pesq_t - 0.009 * wss_m).clamp(1, 5)
    cbak = (1.634 + 0.478 * pesq_t - 0.007 * wss_m + 0.063 * ssnr_m).clamp(1, 5)
    covl = (1.594 + 0.805 * pesq_t - 0.512 * llr_m - 0.007 * wss_m).clamp(1, 5)
    return {'csig': csig, 'cbak': cbak, 'covl': covl, 'pesq': pesq_t, 'ssnr': ssnr_m,
            'wss': wss_m, 'llr': llr_m}


def _same_shape_rows(what, ref, deg):
    ref = _as_rows(ref, 'ref')
    deg = _as_rows(deg, 'deg')
    if ref.shape != deg.shape:
        raise ValueError('{}: ref {} and deg {} differ in shape (signals of different lengths '
                         'are not compared)'.format(what, tuple(ref.shape), tuple(deg.shape)))
    return ref.float().contiguous(), deg.float().contiguous()


def stoi(ref, deg, srate=SRATE, lengths=None):
    """STOI of each row of ref / deg ([rows, T] or [T] CUDA tensors of the same shape) on the
    device: fp64 tensor [rows].  srate: any integer from 4000 to 48000 Hz (resampled to 10 kHz on
    the device).  `lengths`: optional per-row valid sample counts, so that signals of different
    lengths go through one call padded to a common T (row r is ref[r, :lengths[r]]).

    Unlike composite_eval, which truncates to the common length, ref and deg of different
    lengths raise ValueError, as stoi.m does.  NaN where STOI is undefined: a clean signal of
    digital silence, fewer than 30 band frames (about 0.4 s of non-silent speech) or a 0/0
    correlation."""
    return ops.stoi(*_same_shape_rows('stoi', ref, deg), srate, lengths)


def estoi(ref, deg, srate=SRATE, lengths=None):
    """ESTOI (Jensen & Taal's extended STOI, which unlike STOI does not over-rate speech in
    modulated noise such as babble) of each row of ref / deg: the contract of `stoi` (same
    arguments, ValueError for different shapes, fp64 tensor [rows] on the device).  NaN where it
    is undefined: a clean signal of digital silence or fewer than 30 band frames; a degenerate
    band or frame of a window counts as uncorrelated (the zero rule)."""
    return ops.estoi(*_same_shape_rows('estoi', ref, deg), srate, lengths)


def fwsegsnr(ref, deg, srate=SRATE, lengths=None):
    """Frequency-weighted segmental SNR (fwSNRseg) of each row of ref / deg
    ([rows, T] or [T] CUDA tensors of the same shape; `lengths` as for `stoi`) on the device: fp64
    tensor [rows], the mean of the row's finite frame values.  NaN where no frame is finite: fewer
    samples than one frame (T < win + hop, 600 at 16 kHz) or digital silence throughout."""
    return ops.fwsegsnr(*_same_shape_rows('fwsegsnr', ref, deg), srate, lengths)[1]


def cepstral_distance(ref, deg, srate=SRATE, lengths=None):
    """LPC cepstrum distance (CD) of each row of ref / deg (the contract of
    `fwsegsnr`): fp64 tensor [rows], the 0.95-trimmed mean of the row's finite frame values
    (ascending, the first trimmed_count(n_finite) of them).  NaN where no frame is finite."""
    frames = ops.cepstral_distance(*_same_shape_rows('cepstral_distance', ref, deg), srate, lengths)
    rows, nf = frames.shape
    if nf == 0:
        return torch.full((rows,), math.nan, device=frames.device, dtype=torch.float64)
    # NaN sorts last: the first n_finite of each sorted row are its finite values
    srt = torch.sort(frames, dim=1).values
    n_fin = torch.isfinite(frames).sum(dim=1)
    keep = torch.tensor([trimmed_count(n) for n in range(nf + 1)], device=frames.device)[n_fin]
    sel = torch.arange(nf, device=frames.device).unsqueeze(0) < keep.unsqueeze(1)
    total = torch.where(sel, srt, torch.zeros_like(srt)).sum(dim=1)
    return total / keep        # 0 / 0: NaN without a finite frame


def si_sdr(ref, deg, lengths=None):
    """Scale-invariant SDR in dB (Le Roux et al. 2019) of each row of ref / deg (shapes and
    `lengths` as for `stoi`): fp64 tensor [rows].  NaN for a clean signal without energy once its
    mean is removed, +inf where the processed signal is an exact scaled, shifted copy."""
    return ops.si_sdr(*_same_shape_rows('si_sdr', ref, deg), lengths)


def sdr(ref, deg, lengths=None, taps=ops.SDR_TAPS):
    """BSS-eval signal-to-distortion ratio in dB (the SDR of bss_eval_sources, DESIGN.md section
    15) of each row of ref / deg (shapes as for `stoi`; `lengths`: per-row sample counts 0 .. T):
    the processed signal projected onto the clean one and its first taps - 1 delays (taps in
    1 .. 512), the projection's energy over the rest's; fp64 tensor [rows].  Unlike `si_sdr` it
    does not punish a short filter or delay left in the processed signal.  NaN for a row without
    samples, a clean signal without energy or a processed signal of zeros; +inf where the
    processed signal is the clean one times a power of two."""
    return ops.sdr(*_same_shape_rows('sdr', ref, deg), lengths, taps)


def srmr(x, srate=16000, lengths=None):
    """SRMR, the speech-to-reverberation modulation energy ratio (Falk, Zheng and Chan 2010;
    DESIGN.md section 16) of each row of x ([T] or [rows, T], fp32 on the device) at `srate` (16000
    or 8000; `lengths`: per-row sample counts 0 .. T): fp64 tensor [rows], higher is better.  The
    one measure here that needs no clean signal.  NaN for a row shorter than 0.256 s or without
    energy."""
    return ops.srmr(_as_rows(x, 'x').float().contiguous(), lengths, srate)


TRACKERS = ('yin', 'pyin')


def _tracker(tracker):
    if tracker not in TRACKERS:
        raise ValueError('tracker must be one of {}, got {!r}'.format(TRACKERS, tracker))
    return tracker


def _track(x, lengths, srate, threshold, tracker):
    """(f0, lag, ap or vprob, nframes) of ops.pitch or ops.pyin"""
    if tracker == 'pyin':
        return ops.pyin(x, lengths, srate)
    return ops.pitch(x, lengths, srate, threshold)


def pitch(x, srate=16000, lengths=None, threshold=ops.PITCH_THETA, tracker='yin'):
    """The pitch contour of each row of x ([T] or [rows, T], fp32 on the device) at `srate` (16000
    or 8000) by YIN with a 5 ms hop: (f0 fp64 [rows, F] in Hz, 0 where
    unvoiced; voiced bool [rows, F]; ap fp64 [rows, F], the normalised difference at the pick,
    small for a clearly periodic frame).  `lengths`: per-row sample counts 0 .. T; frames from a
    row's own count on are unvoiced with ap = NaN.  A row shorter than 667 samples at 16 kHz has
    no frame.  tracker='pyin': the Viterbi-smoothed contour on the same frames (DESIGN.md section
    22; `threshold` does not apply), and the third value is vprob, the frame's probability of
    being voiced before the decoding."""
    _tracker(tracker)
    f0, lag, ap, _ = _track(_as_rows(x, 'x').float().contiguous(), lengths, srate, threshold,
                            tracker)
    return f0, lag > 0, ap


def f0_eval(ref, deg, srate=SRATE, lengths=None, threshold=ops.PITCH_THETA, tracker='yin'):
    """Whether the processed signal has the clean one's pitch: the F0 / voicing measures of the
    reference's F0Evaluator on the YIN contours (`pitch`) of each row of ref / deg (the argument
    contract of `stoi`: the same shape or ValueError, `lengths` per row), as a dict of fp64 tensors
    [rows]: 'f0_mae' (Hz, over the clean signal's voiced frames), 'vuv_acc' (share of frames with
    the same voiced / unvoiced decision), 'f0_kld' (KL divergence between the Gaussian fits of the
    two log-f0 distributions) and 'voiced' (the clean signal's share of voiced frames).  NaN where
    a measure is undefined: no frame; for f0_mae and f0_kld a signal without a voiced frame
    (DESIGN.md section 19).  The contours are YIN's, not Ahocoder's: the numbers compare systems
    evaluated with this tool, not with tables made with Ahocoder.  tracker='pyin' takes both
    contours from the Viterbi-smoothed tracker, which holds on noisy and
    whispered input where YIN's fixed threshold gives way."""
    _tracker(tracker)
    ref, deg = _same_shape_rows('f0_eval', ref, deg)
    fr, lr, _, nfr = _track(ref, lengths, srate, threshold, tracker)
    fd, ld, _, _ = _track(deg, lengths, srate, threshold, tracker)
    out = ops.f0_eval(fr, lr, fd, ld, nfr)
    return {'f0_mae': out[:, 0], 'vuv_acc': out[:, 1], 'f0_kld': out[:, 2], 'voiced': out[:, 3]}
