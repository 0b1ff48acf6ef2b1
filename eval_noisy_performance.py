"""Composite evaluation (CSIG / CBAK / COVL / PESQ / SSNR) of a directory of degraded wavs against
the clean wavs of the same names, on the MI355X: the reference's eval_noisy_performance.py.

    python eval_noisy_performance.py --test_wavs DIR --clean_wavs DIR --logfile FILE [--stoi]
                                     [--estoi] [--fwsegsnr] [--cd] [--sisdr] [--sdr] [--srmr]
                                     [--f0 [--f0_tracker {yin,pyin}]] [--resample]
                                     [--baseline {wiener,logmmse}]
                                     [--wpe [--wpe_taps K] [--wpe_delay D] [--wpe_iterations I]]
                                     [--omlsa]

16 kHz wavs only (int16 files are scaled by 1/32768, float files used as they are), unless
--resample converts files of other rates to 16 kHz on the GPU first (int16 files to int16, float
files to float32; --resample_zeros / --resample_beta set the filter); PESQ needs
the external `pesqmain` on PATH (NaN, and so NaN CSIG / CBAK / COVL, without it).  --stoi adds
a STOI column (quality.stoi on the GPU, both files truncated to their common length) and a final
mean STOI line; --estoi does the same with an ESTOI column (quality.estoi, extended STOI), after
STOI's when both are given.  --fwsegsnr, --cd and --sisdr add, in that order after them, the
columns FWSEGSNR (quality.fwsegsnr, frequency-weighted segmental SNR in dB), CD
(quality.cepstral_distance, LPC cepstrum distance) and SISDR (quality.si_sdr, scale-invariant SDR
in dB) with their final mean lines; none of the three needs pesqmain.  --sdr adds, after them, the
column SDR (quality.sdr, the BSS-eval signal-to-distortion ratio in dB with a 512-tap distortion
filter) and its mean line.  --srmr adds, last, the column SRMR (quality.srmr, the
speech-to-reverberation modulation energy ratio of the degraded file alone: it needs no clean
signal) and its mean line.  --f0 adds, after every other column, F0MAE, VUV and F0KLD
(quality.f0_eval: the F0 mean absolute error in Hz, the voiced / unvoiced accuracy and the KL
divergence between the log-F0 distributions, on YIN contours tracked on the GPU) and, for each, a
final mean line over the files where it is finite with the count of NaN files; --f0_tracker pyin
takes the contours from the Viterbi-smoothed tracker instead (same columns).  --baseline
{wiener,logmmse} passes every degraded file through that statistical-model enhancer
(segan_pytorch_amd.baselines, at 16 kHz, float32) before all measures, so that one run gives the
baseline's row of a results table; the header line and the columns are unchanged.  --wpe passes
every degraded file through the WPE dereverberator (baselines.wpe, at 16 kHz, float32; --wpe_taps,
--wpe_delay, --wpe_iterations) before all measures, and before the --baseline enhancer if both are
given; the header line and the columns are unchanged as well.  --omlsa passes every degraded file
through the OM-LSA enhancer with IMCRA noise tracking (baselines.omlsa, at 16 kHz, float32) before
all measures, after --wpe if both are given; with --baseline it is refused; the header line and the
columns are unchanged."""
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


# the optional columns in their order: (column, flag, function of segan_pytorch_amd.quality)
EXTRA = (('STOI', 'stoi', 'stoi'), ('ESTOI', 'estoi', 'estoi'),
         ('FWSEGSNR', 'fwsegsnr', 'fwsegsnr'), ('CD', 'cd', 'cepstral_distance'),
         ('SISDR', 'sisdr', 'si_sdr'), ('SDR', 'sdr', 'sdr'), ('SRMR', 'srmr', 'srmr'))
BLIND = ('SRMR',)     # columns computed on the degraded file alone
# the columns of --f0, after every column of EXTRA: (column, key of quality.f0_eval's dict)
F0_COLUMNS = (('F0MAE', 'f0_mae'), ('VUV', 'vuv_acc'), ('F0KLD', 'f0_kld'))


def header_line(opts):
    return 'FILE CSIG CBAK COVL PESQ SSNR' + ''.join(
        ' ' + name for name, flag, _ in EXTRA if getattr(opts, flag)) + ''.join(
            ' ' + name for name, _ in F0_COLUMNS if getattr(opts, 'f0', False))


def main(opts):
    from segan_pytorch_amd.baselines import omlsa_opts
    omlsa = omlsa_opts(opts)         # refuses --omlsa with --baseline before any device is asked for
    if not torch.cuda.is_available():
        raise SystemExit('segan_pytorch_amd runs only on an MI355X (HIP) device; pass --cuda on a '
                         'GPU machine (there is no CPU fallback)')
    from segan_pytorch_amd import baselines, quality
    from segan_pytorch_amd.quality import composite_eval
    baseline = getattr(opts, 'baseline', None)
    wpe = baselines.wpe_opts(opts)
    extra = [(name, getattr(quality, fn)) for name, flag, fn in EXTRA if getattr(opts, flag)]
    noisy_wavs = sorted(glob.glob(os.path.join(opts.test_wavs, '*.wav')))
    metrics = {'csig': [], 'cbak': [], 'covl': [], 'STOI': [], 'ESTOI': [], 'FWSEGSNR': [],
               'CD': [], 'SISDR': [], 'SDR': [], 'SRMR': []}
    with_f0 = bool(getattr(opts, 'f0', False))
    f0_rows = {name: [] for name, _ in F0_COLUMNS}
    timings = []
    with open(opts.logfile, 'w') as out_log:
        out_log.write(header_line(opts) + '\n')
        for n_i, noisy_wav in enumerate(noisy_wavs, start=1):
            bname = os.path.splitext(os.path.basename(noisy_wav))[0]
            clean_wav = os.path.join(opts.clean_wavs, bname + '.wav')
            noisy = read_wav(noisy_wav, opts)
            clean = read_wav(clean_wav, opts)
            if wpe is not None:
                noisy = baselines.wpe(torch.from_numpy(noisy).cuda(), **wpe).cpu().numpy()
            if baseline is not None:
                noisy = baselines.denoise(torch.from_numpy(noisy).cuda(),
                                          rule=baseline).cpu().numpy()
            if omlsa:
                noisy = baselines.omlsa(torch.from_numpy(noisy).cuda()).cpu().numpy()
            beg_t = timeit.default_timer()
            r = composite_eval(torch.from_numpy(clean).cuda(), torch.from_numpy(noisy).cuda())
            csig, cbak, covl, pesq, ssnr = (float(r[k][0]) for k in
                                            ('csig', 'cbak', 'covl', 'pesq', 'ssnr'))
            if extra:
                L = min(len(clean), len(noisy))
                c, d = torch.from_numpy(clean[:L]).cuda(), torch.from_numpy(noisy[:L]).cuda()
                for name, fn in extra:
                    if name in BLIND:
                        metrics[name].append(float(fn(torch.from_numpy(noisy).cuda())[0]))
                    else:
                        metrics[name].append(float(fn(c, d)[0]))
            if with_f0:
                L = min(len(clean), len(noisy))
                f0r = quality.f0_eval(torch.from_numpy(clean[:L]).cuda(),
                                      torch.from_numpy(noisy[:L]).cuda(),
                                      tracker=getattr(opts, 'f0_tracker', 'yin'))
                for name, key in F0_COLUMNS:
                    f0_rows[name].append(float(f0r[key][0]))
            end_t = timeit.default_timer()
            timings.append(end_t - beg_t)
            metrics['csig'].append(csig)
            metrics['cbak'].append(cbak)
            metrics['covl'].append(covl)
            out_log.write('{} {:.3f} {:.3f} {:.3f} {:.3f} {:.3}'.format(bname + '.wav', csig,
                                                                        cbak, covl, pesq, ssnr) +
                          ''.join(' {:.4f}'.format(metrics[name][-1]) for name, _ in extra) +
                          ''.join(' {:.4f}'.format(f0_rows[name][-1]) for name, _ in F0_COLUMNS
                                  if with_f0) + '\n')
            print('Processed {}/{} wav, CSIG:{:.3f} CBAK:{:.3f} COVL:{:.3f} '
                  'PESQ:{:.3f} SSNR:{:.3f} '
                  'total time: {:.2f} seconds, mproc: {:.2f}'
                  ' seconds'.format(n_i, len(noisy_wavs), csig, cbak, covl, pesq, ssnr,
                                    np.sum(timings), np.mean(timings)))
    print('mean Csig: ', np.mean(metrics['csig']))
    print('mean Cbak: ', np.mean(metrics['cbak']))
    print('mean Covl: ', np.mean(metrics['covl']))
    for name, _ in extra:
        print('mean {}: '.format(name), np.mean(metrics[name]))
    if with_f0:
        for name, _ in F0_COLUMNS:
            v = np.asarray(f0_rows[name], dtype=np.float64)
            fin = v[np.isfinite(v)]
            print('mean {}: '.format(name), fin.mean() if len(fin) else float('nan'),
                  '({} NaN of {} files)'.format(len(v) - len(fin), len(v)))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('--test_wavs', type=str, required=True)
    parser.add_argument('--clean_wavs', type=str, required=True)
    parser.add_argument('--logfile', type=str, required=True)
    parser.add_argument('--stoi', action='store_true', default=False,
                        help='also compute STOI (short-time objective intelligibility)')
    parser.add_argument('--estoi', action='store_true', default=False,
                        help='also compute ESTOI (extended STOI, the measure for modulated '
                             'noise such as babble)')
    parser.add_argument('--fwsegsnr', action='store_true', default=False,
                        help='also compute fwSNRseg (frequency-weighted segmental SNR, dB)')
    parser.add_argument('--cd', action='store_true', default=False,
                        help='also compute CD (LPC cepstrum distance)')
    parser.add_argument('--sisdr', action='store_true', default=False,
                        help='also compute SI-SDR (scale-invariant signal-to-distortion ratio, dB)')
    parser.add_argument('--sdr', action='store_true', default=False,
                        help='also compute SDR (BSS-eval signal-to-distortion ratio with a '
                             '512-tap distortion filter, dB)')
    parser.add_argument('--srmr', action='store_true', default=False,
                        help='also compute SRMR (speech-to-reverberation modulation energy ratio '
                             'of the degraded file alone)')
    parser.add_argument('--f0', action='store_true', default=False,
                        help='also compute F0MAE, VUV and F0KLD (F0 mean absolute error in Hz, '
                             'voiced / unvoiced accuracy, KL divergence of the log-F0 '
                             'distributions) on YIN pitch contours')
    parser.add_argument('--f0_tracker', choices=('yin', 'pyin'), default='yin',
                        help='the pitch tracker behind --f0: plain YIN, or pyin, its '
                             'Viterbi-smoothed form, which holds on noisy and whispered input '
                             '(the columns are the same)')
    parser.add_argument('--baseline', choices=('wiener', 'logmmse'), default=None,
                        help='enhance every degraded file with this statistical-model baseline '
                             'before all measures')
    parser.add_argument('--resample', action='store_true', default=False,
                        help='convert wavs that are not 16 kHz to 16 kHz on the GPU instead of '
                             'refusing them')
    from segan_pytorch_amd.baselines import add_omlsa_flags, add_wpe_flags
    from segan_pytorch_amd.resample import add_filter_flags
    add_filter_flags(parser)
    add_wpe_flags(parser)
    add_omlsa_flags(parser)
    return parser


if __name__ == '__main__':
    main(build_parser().parse_args())
