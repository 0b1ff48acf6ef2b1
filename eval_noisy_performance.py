"""Composite evaluation (CSIG / CBAK / COVL / PESQ / SSNR) of a directory of degraded wavs against
the clean wavs of the same names, on the MI355X: the reference's eval_noisy_performance.py.

    python eval_noisy_performance.py --test_wavs DIR --clean_wavs DIR --logfile FILE [--stoi]
                                     [--resample]

16 kHz wavs only (int16 files are scaled by 1/32768, float files used as they are), unless
--resample converts files of other rates to 16 kHz on the GPU first (int16 files to int16, float
files to float32; --resample_zeros / --resample_beta set the filter); PESQ needs
the external `pesqmain` on PATH (NaN, and so NaN CSIG / CBAK / COVL, without it).  --stoi adds
a STOI column (quality.stoi on the GPU, both files truncated to their common length) and a final
mean STOI line."""
import argparse
import glob
import os
import sys
import timeit

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def read_wav(path, opts=None):
    from scipy.io import wavfile
    rate, x = wavfile.read(path)
    if rate != 16000 and getattr(opts, 'resample', False):
        from segan_pytorch_amd.resample import resample_wav
        try:
            x = resample_wav(x, rate, 16000, opts.resample_zeros, opts.resample_beta)
        except (TypeError, ValueError, RuntimeError) as e:
            raise SystemExit('{}: {}'.format(path, e))
    elif rate != 16000:
        raise SystemExit('{}: sample rate {} Hz; only 16 kHz wavs are supported (no '
                         'resampling)'.format(path, rate))
    if x.dtype == np.int16:
        x = x.astype(np.float32) / 32768
    elif np.issubdtype(x.dtype, np.floating):
        x = x.astype(np.float32)
    else:
        raise SystemExit('{}: unsupported sample format {}'.format(path, x.dtype))
    if x.ndim > 1:
        x = x.mean(axis=1, dtype=np.float32)
    return x


def main(opts):
    if not torch.cuda.is_available():
        raise SystemExit('segan_pytorch_amd runs only on an MI355X (HIP) device; pass --cuda on a '
                         'GPU machine (there is no CPU fallback)')
    from segan_pytorch_amd.quality import composite_eval, stoi
    noisy_wavs = sorted(glob.glob(os.path.join(opts.test_wavs, '*.wav')))
    metrics = {'csig': [], 'cbak': [], 'covl': [], 'stoi': []}
    timings = []
    with open(opts.logfile, 'w') as out_log:
        out_log.write('FILE CSIG CBAK COVL PESQ SSNR' + (' STOI' if opts.stoi else '') + '\n')
        for n_i, noisy_wav in enumerate(noisy_wavs, start=1):
            bname = os.path.splitext(os.path.basename(noisy_wav))[0]
            clean_wav = os.path.join(opts.clean_wavs, bname + '.wav')
            noisy = read_wav(noisy_wav, opts)
            clean = read_wav(clean_wav, opts)
            beg_t = timeit.default_timer()
            r = composite_eval(torch.from_numpy(clean).cuda(), torch.from_numpy(noisy).cuda())
            csig, cbak, covl, pesq, ssnr = (float(r[k][0]) for k in
                                            ('csig', 'cbak', 'covl', 'pesq', 'ssnr'))
            if opts.stoi:
                L = min(len(clean), len(noisy))
                metrics['stoi'].append(float(stoi(torch.from_numpy(clean[:L]).cuda(),
                                                  torch.from_numpy(noisy[:L]).cuda())[0]))
            end_t = timeit.default_timer()
            timings.append(end_t - beg_t)
            metrics['csig'].append(csig)
            metrics['cbak'].append(cbak)
            metrics['covl'].append(covl)
            out_log.write('{} {:.3f} {:.3f} {:.3f} {:.3f} {:.3}'.format(bname + '.wav', csig,
                                                                        cbak, covl, pesq, ssnr) +
                          (' {:.4f}'.format(metrics['stoi'][-1]) if opts.stoi else '') + '\n')
            print('Processed {}/{} wav, CSIG:{:.3f} CBAK:{:.3f} COVL:{:.3f} '
                  'PESQ:{:.3f} SSNR:{:.3f} '
                  'total time: {:.2f} seconds, mproc: {:.2f}'
                  ' seconds'.format(n_i, len(noisy_wavs), csig, cbak, covl, pesq, ssnr,
                                    np.sum(timings), np.mean(timings)))
    print('mean Csig: ', np.mean(metrics['csig']))
    print('mean Cbak: ', np.mean(metrics['cbak']))
    print('mean Covl: ', np.mean(metrics['covl']))
    if opts.stoi:
        print('mean STOI: ', np.mean(metrics['stoi']))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--test_wavs', type=str, required=True)
    parser.add_argument('--clean_wavs', type=str, required=True)
    parser.add_argument('--logfile', type=str, required=True)
    parser.add_argument('--stoi', action='store_true', default=False,
                        help='also compute STOI (short-time objective intelligibility)')
    parser.add_argument('--resample', action='store_true', default=False,
                        help='convert wavs that are not 16 kHz to 16 kHz on the GPU instead of '
                             'refusing them')
    from segan_pytorch_amd.resample import add_filter_flags
    add_filter_flags(parser)
    return parser


if __name__ == '__main__':
    main(build_parser().parse_args())
