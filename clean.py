#!/usr/bin/env python
"""Enhance wav files with a trained generator — the reference's clean.py entry point
(same flags; reads the `train.opts` written by train.py and a generator checkpoint) on
the HIP path.

    python clean.py --g_pretrained_ckpt ckpt/weights_EOE_G-Generator-N.ckpt \
        --cfg_file ckpt/train.opts --test_files noisy_dir --synthesis_path out --cuda

Files are taken as 16 kHz whatever their header says, as in the reference, unless --resample is
given: a file of another rate is then converted to 16 kHz int16 on the GPU first (the reference
leans on librosa.load(path, 16000) or an offline sox pass), and with --keep_rate the enhanced
signal is converted back and written at the file's own rate and length.  --srmr prints the SRMR
(quality.srmr, the speech-to-reverberation modulation energy ratio, which needs no clean signal)
of each enhanced signal at 16 kHz and the mean over the files.

    python clean.py --baseline logmmse --test_files noisy_dir --synthesis_path out --cuda

--baseline {wiener,logmmse} enhances with a statistical-model baseline (segan_pytorch_amd.baselines)
instead of a generator: no --cfg_file and no checkpoint, no normalisation and no pre-emphasis; an
int16 file is written as int16 (rounded, clipped), any other as float32.  --resample, --keep_rate
and --srmr apply as above.

    python clean.py --wpe --test_files reverberant_dir --synthesis_path out --cuda

--wpe dereverberates with WPE (weighted prediction error, baselines.wpe_wav; --wpe_taps,
--wpe_delay and --wpe_iterations set its 10 taps, delay of 3 frames and 3 iterations).  Alone it
works like --baseline: no --cfg_file, no checkpoint, no normalisation.  With --baseline RULE the
file goes through WPE first and the denoiser after it, the usual chain on reverberant and noisy
speech.  With --cfg_file it is refused: a generator is trained on its own input.

    python clean.py --omlsa --test_files noisy_dir --synthesis_path out --cuda

--omlsa enhances with OM-LSA on an IMCRA noise estimate (baselines.omlsa_wav), which follows a
noise level that changes and takes no noise segment from the start of the file.  It works like
--baseline (no --cfg_file, no checkpoint, no normalisation), runs after --wpe if both are given,
and is refused together with --baseline or --cfg_file.
"""
import argparse
import glob
import json
import os
import random
import timeit
from types import SimpleNamespace

import numpy as np
import torch
from scipy.io import wavfile

from segan_pytorch_amd import baselines
from segan_pytorch_amd.datasets import normalize_wave_minmax, pre_emphasize
from segan_pytorch_amd.models import SEGAN, WSEGAN
from segan_pytorch_amd.ops import RESAMPLE_BETA, RESAMPLE_ZEROS
from segan_pytorch_amd.resample import TARGET_RATE, as_mono, resample_wav

BASELINES = ('wiener', 'logmmse')


def build_parser():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument('--g_pretrained_ckpt', type=str, default=None)
    p.add_argument('--test_files', type=str, nargs='+', default=None)
    p.add_argument('--h5', action='store_true', default=False)
    p.add_argument('--seed', type=int, default=111)
    p.add_argument('--synthesis_path', type=str, default='segan_samples')
    p.add_argument('--cuda', action='store_true', default=False)
    p.add_argument('--soundfile', action='store_true', default=False)
    p.add_argument('--cfg_file', type=str, default=None)
    # additions over the reference: absent from the namespace unless given (argparse.SUPPRESS), so
    # the default namespace stays the reference's eight flags; read them through resample_opts()
    p.add_argument('--resample', action='store_true', default=argparse.SUPPRESS,
                   help='convert files that are not 16 kHz to 16 kHz int16 on the GPU before '
                        'enhancing them (without it the rate in the header is ignored)')
    p.add_argument('--keep_rate', action='store_true', default=argparse.SUPPRESS,
                   help='implies --resample; convert the enhanced signal back to the file\'s rate, '
                        'trim it to the file\'s length and write it at that rate')
    p.add_argument('--resample_zeros', type=int, default=argparse.SUPPRESS,
                   help='zero crossings a side of the conversion filter (default {}; 10 with '
                        '--resample_beta 5.0 is scipy\'s default)'.format(RESAMPLE_ZEROS))
    p.add_argument('--resample_beta', type=float, default=argparse.SUPPRESS,
                   help='Kaiser beta of the conversion filter (default {})'.format(RESAMPLE_BETA))
    p.add_argument('--srmr', action='store_true', default=argparse.SUPPRESS,
                   help='print the SRMR (speech-to-reverberation modulation energy ratio) of each '
                        'enhanced signal at 16 kHz, and the mean')
    p.add_argument('--baseline', choices=BASELINES, default=argparse.SUPPRESS,
                   help='enhance with this statistical-model baseline instead of a generator; '
                        'needs neither --cfg_file nor --g_pretrained_ckpt')
    baselines.add_wpe_flags(p)
    baselines.add_omlsa_flags(p)
    return p


def resample_opts(opts):
    """(resample, keep_rate, zeros, beta) of a parsed namespace; keep_rate implies resample."""
    keep = getattr(opts, 'keep_rate', False)
    return (getattr(opts, 'resample', False) or keep, keep,
            getattr(opts, 'resample_zeros', RESAMPLE_ZEROS), getattr(opts, 'resample_beta', RESAMPLE_BETA))


def main(opts):
    resample, keep_rate, rs_zeros, rs_beta = resample_opts(opts)
    baseline = getattr(opts, 'baseline', None)
    wpe = baselines.wpe_opts(opts)
    if wpe is not None and opts.cfg_file is not None:
        raise SystemExit('--wpe does not go with --cfg_file: it runs alone or before --baseline, '
                         'not in front of a generator')
    omlsa = baselines.omlsa_opts(opts)
    if omlsa and opts.cfg_file is not None:
        raise SystemExit('--omlsa does not go with --cfg_file: it is an enhancer of its own')
    classical = baseline is not None or wpe is not None or omlsa
    if classical:
        if opts.test_files is None:
            raise SystemExit('--test_files is required')
    elif opts.cfg_file is None or opts.test_files is None or opts.g_pretrained_ckpt is None:
        raise SystemExit('--cfg_file, --test_files and --g_pretrained_ckpt are required')
    if not (opts.cuda and torch.cuda.is_available()):
        raise SystemExit('segan_pytorch_amd runs only on an MI355X (HIP) device; pass --cuda on a '
                         'GPU machine (there is no CPU fallback)')
    if opts.h5:
        raise NotImplementedError('--h5 input is not implemented')
    if not classical:
        with open(opts.cfg_file, 'r') as f:
            cfg = json.load(f)
        cfg.setdefault('reg_loss', 'l1_loss')      # older train.opts predate this flag
        args = SimpleNamespace(**cfg)
        args.cuda = True
        segan = (WSEGAN if getattr(args, 'wsegan', False) else SEGAN)(args)
        segan.G.load_pretrained(opts.g_pretrained_ckpt, True)
        segan.cuda()
        segan.G.eval()
    if len(opts.test_files) == 1 and os.path.isdir(opts.test_files[0]):
        twavs = sorted(glob.glob(os.path.join(opts.test_files[0], '*.wav')))
    else:
        twavs = opts.test_files
    print('Cleaning {} wavs'.format(len(twavs)))
    with_srmr, srmrs = getattr(opts, 'srmr', False), []
    beg_t = timeit.default_timer()
    for t_i, twav in enumerate(twavs, start=1):
        rate, wav = wavfile.read(twav)
        n_in = wav.shape[0]
        convert = resample and rate != TARGET_RATE
        if convert:
            wav = resample_wav(wav, rate, TARGET_RATE, rs_zeros, rs_beta)
        out_path = os.path.join(opts.synthesis_path, os.path.basename(twav))
        if not classical:
            wav = pre_emphasize(normalize_wave_minmax(wav), args.preemph)
            pwav = torch.as_tensor(wav, dtype=torch.float32).view(1, 1, -1).cuda()
            g_wav, _g_c = segan.generate(pwav, device='cuda')
            g_wav, out_rate = np.asarray(g_wav, dtype=np.float32), int(16e3)
        else:
            g_wav, out_rate = as_mono(wav), int(16e3)
            if wpe is not None:
                g_wav = baselines.wpe_wav(g_wav, **wpe)
            if baseline is not None:
                g_wav = baselines.denoise_wav(g_wav, baseline)
            if omlsa:
                g_wav = baselines.omlsa_wav(g_wav)
        if with_srmr:
            from segan_pytorch_amd import quality
            f_wav = g_wav / 32768 if g_wav.dtype == np.int16 else g_wav
            f_wav = np.asarray(f_wav, dtype=np.float32).reshape(-1)
            srmrs.append(float(quality.srmr(torch.from_numpy(f_wav).cuda())[0]))
        if convert and keep_rate:
            g_wav = resample_wav(g_wav.reshape(-1), TARGET_RATE, rate, rs_zeros, rs_beta)[:n_in]
            out_rate = rate
        wavfile.write(out_path, out_rate, g_wav)
        end_t = timeit.default_timer()
        print('Cleaned {}/{}: {} in {} s'.format(t_i, len(twavs), twav, end_t - beg_t))
        if with_srmr:
            print('SRMR {}: {:.4f}'.format(out_path, srmrs[-1]))
        beg_t = timeit.default_timer()
    if with_srmr:
        print('mean SRMR: ', np.nanmean(srmrs) if srmrs else float('nan'))


if __name__ == '__main__':
    opts = build_parser().parse_args()
    os.makedirs(opts.synthesis_path, exist_ok=True)
    random.seed(opts.seed)
    np.random.seed(opts.seed)
    torch.manual_seed(opts.seed)
    main(opts)
