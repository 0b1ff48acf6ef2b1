#!/usr/bin/env python
"""Train SEGAN+ / WSEGAN on MI355X — the reference's train.py entry point (same flags,
same defaults, same `train.opts` dump) driving the HIP engine in `segan_pytorch_amd`.

    python train.py --save_path ckpt_segan+ --clean_trainset ... --noisy_trainset ... \
        --batch_size 300 --no_train_gen
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 train.py ...

Additions over the reference: `--synthetic N` trains on N fixed-seed synthetic chunk
pairs (no dataset needed), `--pcm_shard PREFIX` trains from a pre-sliced int16 shard whose
batches are normalised / pre-emphasised on the GPU (with `--additive_noises DIR` noise is mixed
into them on the fly at `--additive_snrs` dB, the reference's Additive; with `--reverb_rirs DIR`
each selected clean slice is first convolved on the GPU with a room impulse response drawn from
DIR's wavs: `--reverb_prob` is the share of items selected, `--reverb_max_taps` cuts the
responses, `--reverb_resample` converts responses that are not 16 kHz, and `--reverb_synth N` synthesises
N responses of shoebox rooms on the GPU instead of, or after, DIR's: `--reverb_rt60 LO HI`,
`--reverb_room_min X Y Z` and `--reverb_room_max X Y Z` bound the rooms drawn; with `--distort KIND ...`
each selected item (`--distort_prob`) is then clipped, has chunks of speech removed or is band
limited on the GPU, one kind per item drawn from `clip chop bandlimit`: `--clip_factors`,
`--chop_max`, `--chop_durs LO HI` and `--bandlimit_cutoffs` set the kinds' parameters, and
'_clip' / '_chop' / '_bandlimit' is appended to the item's name; with `--whisper` each selected
item (`--whisper_prob`) is first of all turned into pseudo-whisper on the GPU by noise-excited LPC
resynthesis, with a spectral tilt drawn from `--whisper_tilts` and an envelope smoothed by
`--whisper_lag_hz`, while the clean, voiced slice stays the target), and under
torch.distributed.run every
rank trains on its shard of each epoch with RCCL gradient averaging.
"""
import argparse
import json
import os
import random

import numpy as np
import torch
from torch.utils.data import DataLoader

from segan_pytorch_amd import distributed as sdist
from segan_pytorch_amd import losses
from segan_pytorch_amd.datasets import (PCMShardCollate, PCMShardDataset, SEDataset,
                                        SyntheticSEDataset, collate_fn)
from segan_pytorch_amd.models import SEGAN, WSEGAN

_FMAPS = [64, 128, 256, 512, 1024]
_POOLS = [4, 4, 4, 4, 4]

# the defaults of the --distort kinds (augment.Clip / Chop / BandLimit)
DISTORT_KINDS = ('clip', 'chop', 'bandlimit')
CLIP_FACTORS = (0.1, 0.2, 0.3, 0.4, 0.5)
CHOP_MAX = 3
CHOP_DURS = (0.05, 0.3)
BANDLIMIT_CUTOFFS = (1000.0, 2000.0, 4000.0)
DISTORT_SRATE = 16000
DISTORT_ZEROS = 32          # augment.lowpass_bank: K = ceil(zeros srate / (2 fc)) taps a side
DISTORT_MAX_K = 2048        # ops.FIR_MAX_K
# the defaults of --whisper (augment.Whisper)
WHISPER_TILTS = (0.0, 0.5, 0.9)
WHISPER_LAG_HZ = 120.0
WHISPER_MAX_LAG_HZ = 1000.0
# the defaults of --reverb_synth (augment.draw_rooms)
REVERB_RT60 = (0.2, 0.8)
REVERB_ROOM_MIN = (3.0, 3.0, 2.5)
REVERB_ROOM_MAX = (10.0, 8.0, 4.0)
REVERB_ROOM_SMALLEST = 2.0  # metres: source and receiver keep 0.5 m from every wall

# (flag, kwargs) — names and defaults are the reference's (train.py:101-247)
FLAGS = [
    ('--save_path', dict(type=str, default='seganv1_ckpt')),
    ('--d_pretrained_ckpt', dict(type=str, default=None)),
    ('--g_pretrained_ckpt', dict(type=str, default=None)),
    ('--cache_dir', dict(type=str, default='data_cache')),
    ('--clean_trainset', dict(type=str, default='data/clean_trainset')),
    ('--noisy_trainset', dict(type=str, default='data/noisy_trainset')),
    ('--clean_valset', dict(type=str, default=None)),
    ('--noisy_valset', dict(type=str, default=None)),
    ('--h5_data_root', dict(type=str, default=None)),
    ('--h5', dict(action='store_true', default=False)),
    ('--data_stride', dict(type=float, default=0.5)),
    ('--seed', dict(type=int, default=111)),
    ('--epoch', dict(type=int, default=100)),
    ('--patience', dict(type=int, default=100)),
    ('--batch_size', dict(type=int, default=100)),
    ('--save_freq', dict(type=int, default=50)),
    ('--slice_size', dict(type=int, default=16384)),
    ('--opt', dict(type=str, default='rmsprop')),
    ('--l1_dec_epoch', dict(type=int, default=100)),
    ('--l1_weight', dict(type=float, default=100)),
    ('--l1_dec_step', dict(type=float, default=1e-5)),
    ('--g_lr', dict(type=float, default=0.00005)),
    ('--d_lr', dict(type=float, default=0.00005)),
    ('--preemph', dict(type=float, default=0.95)),
    ('--max_samples', dict(type=int, default=None)),
    ('--eval_workers', dict(type=int, default=2)),
    ('--eval_stoi', dict(action='store_true', default=False,
                         help='the evaluation also reports STOI (short-time objective '
                              'intelligibility); the validation objective stays SSNR')),
    ('--eval_estoi', dict(action='store_true', default=False,
                          help='the evaluation also reports ESTOI (extended STOI, the measure '
                               'to read beside PESQ under modulated noise such as babble); the '
                               'validation objective stays SSNR')),
    ('--eval_fwsegsnr', dict(action='store_true', default=False,
                             help='the evaluation also reports fwSNRseg (frequency-weighted '
                                  'segmental SNR); the validation objective stays SSNR')),
    ('--eval_cd', dict(action='store_true', default=False,
                       help='the evaluation also reports CD (LPC cepstrum distance)')),
    ('--eval_sisdr', dict(action='store_true', default=False,
                          help='the evaluation also reports SI-SDR (scale-invariant SDR)')),
    ('--eval_sdr', dict(action='store_true', default=False,
                        help='the evaluation also reports SDR (BSS-eval signal-to-distortion '
                             'ratio with a 512-tap distortion filter)')),
    ('--eval_srmr', dict(action='store_true', default=False,
                         help='the evaluation also reports SRMR (speech-to-reverberation '
                              'modulation energy ratio; needs no clean signal)')),
    ('--eval_f0', dict(action='store_true', default=False,
                       help='the evaluation also reports the F0 mean absolute error, the voiced / '
                            'unvoiced accuracy and the log-F0 KL divergence (f0_mae, vuv_acc, '
                            'f0_kld) on YIN pitch contours; the validation objective stays '
                            'SSNR')),
    ('--eval_f0_tracker', dict(choices=('yin', 'pyin'), default='yin',
                               help='the pitch tracker behind --eval_f0: plain YIN, or pyin, its '
                                    'Viterbi-smoothed form (the keys are the same)')),
    ('--slice_workers', dict(type=int, default=1)),
    ('--num_workers', dict(type=int, default=1)),
    ('--no-cuda', dict(action='store_true', default=False)),
    ('--random_scale', dict(type=float, nargs='+', default=[1])),
    ('--no_train_gen', dict(action='store_true', default=False)),
    ('--preemph_norm', dict(action='store_true', default=False)),
    ('--wsegan', dict(action='store_true', default=False)),
    ('--aewsegan', dict(action='store_true', default=False)),
    ('--vanilla_gan', dict(action='store_true', default=False)),
    ('--no_bias', dict(action='store_true', default=False)),
    ('--n_fft', dict(type=int, default=2048)),
    ('--reg_loss', dict(type=str, default='l1_loss')),
    ('--skip_merge', dict(type=str, default='concat')),
    ('--skip_type', dict(type=str, default='alpha')),
    ('--skip_init', dict(type=str, default='one')),
    ('--skip_kwidth', dict(type=int, default=11)),
    ('--gkwidth', dict(type=int, default=31)),
    ('--genc_fmaps', dict(type=int, nargs='+', default=list(_FMAPS))),
    ('--genc_poolings', dict(type=int, nargs='+', default=list(_POOLS))),
    ('--z_dim', dict(type=int, default=1024)),
    ('--gdec_fmaps', dict(type=int, nargs='+', default=None)),
    ('--gdec_poolings', dict(type=int, nargs='+', default=None)),
    ('--gdec_kwidth', dict(type=int, default=None)),
    ('--gnorm_type', dict(type=str, default=None)),
    ('--no_z', dict(action='store_true', default=False)),
    ('--no_skip', dict(action='store_true', default=False)),
    ('--pow_weight', dict(type=float, default=0.001)),
    ('--misalign_pair', dict(action='store_true', default=False)),
    ('--interf_pair', dict(action='store_true', default=False)),
    ('--denc_fmaps', dict(type=int, nargs='+', default=list(_FMAPS))),
    ('--dpool_type', dict(type=str, default='none')),
    ('--dpool_slen', dict(type=int, default=16)),
    ('--dkwidth', dict(type=int, default=None)),
    ('--denc_poolings', dict(type=int, nargs='+', default=list(_POOLS))),
    ('--dnorm_type', dict(type=str, default='bnorm')),
    ('--phase_shift', dict(type=int, default=5)),
    ('--sinc_conv', dict(action='store_true', default=False)),
    # ---- additions ----
    ('--synthetic', dict(type=int, default=0,
                         help='train on this many fixed-seed synthetic chunk pairs')),
    ('--sync_bn', dict(action='store_true', default=False,
                       help='data parallel: take D\'s BatchNorm statistics over the global batch '
                            '(N ranks of batch b behave like one process at batch N*b)')),
    ('--device_z', dict(action='store_true', default=False,
                        help='draw the generator\'s z on the GPU (per-rank generator) instead of on the '
                             'host like the reference (generator.py:197): no host randn + copy per step, '
                             'but not the reference\'s RNG stream')),
    ('--precision', dict(type=str, default=None, choices=['fp32', 'bf16x3', 'bf16'],
                         help='contraction precision of the conv / deconv kernels (default: $SEGAN_PRECISION '
                              'or fp32 = exact fp32 MFMA).  bf16 = mixed precision on the bf16 matrix cores '
                              '(BASELINE config 5: bf16 operands, fp32 accumulation, everything else fp32; '
                              'tolerances in DESIGN.md section 6); bf16x3 = fp32 operands split exactly into '
                              '3 bf16 planes (fp32-class results).  With bf16 z is drawn on the GPU by default '
                              '(--device_z): a step takes about as long as the single-threaded host randn of '
                              'one z, so the host draw would be the critical path; --host_z keeps it')),
    ('--host_z', dict(action='store_true', default=False,
                      help='with --precision bf16: draw z on the host like the reference anyway')),
    ('--no_prefetch_z', dict(action='store_true', default=False,
                             help='draw every z inside its own step instead of one step ahead on a host '
                                  'thread (same numbers either way as long as nothing else takes from torch\'s global CPU '
                                  'generator inside an epoch; if something does — a num_workers=0 dataset using '
                                  'torch RNG, a hook — it is detected and the look-ahead switches itself off '
                                  'with a warning: Generator._host_z)')),
    ('--deterministic', dict(action='store_true', default=False,
                             help='bit-reproducible kernels: the weight-gradient and dense-head contraction '
                                  'splits are added in a fixed order instead of with fp32 atomics '
                                  '(1-2 %% slower)')),
    ('--pcm_shard', dict(type=str, default=None,
                         help='prefix of a pre-sliced int16 shard (scripts/make_pcm_shard.py): batches '
                              'are normalised and pre-emphasised on the GPU')),
    ('--additive_noises', dict(type=str, default=None,
                               help='with --pcm_shard: directory of noise wavs; the noisy row of '
                                    'each selected item is replaced by clean + noise mixed on the '
                                    'GPU at an SNR over the P.56 active speech level (the '
                                    'reference\'s Additive), and \'_additive\' is appended to its '
                                    'utterance name')),
    ('--additive_snrs', dict(type=float, nargs='+', default=[0, 5, 10],
                             help='SNR levels in dB drawn uniformly per item')),
    ('--additive_prob', dict(type=float, default=1.0,
                             help='probability that an item is mixed on the fly')),
    ('--additive_resample', dict(action='store_true', default=False,
                                 help='with --additive_noises: convert noise wavs that are not '
                                      '16 kHz (the DEMAND noises are 48 kHz) to 16 kHz on the GPU '
                                      'when they are read; without it their rate is ignored')),
    ('--reverb_rirs', dict(type=str, default=None,
                           help='with --pcm_shard: directory of room impulse response wavs; the '
                                'clean wave of each selected item is convolved on the GPU with one '
                                'of them (direct path aligned with the dry target, gain 1) before '
                                'any noise is mixed, and \'_reverb\' is appended to its utterance '
                                'name')),
    ('--reverb_prob', dict(type=float, default=1.0,
                           help='probability that an item is reverberated')),
    ('--reverb_max_taps', dict(type=int, default=16384,
                               help='impulse responses are cut to this many taps')),
    ('--reverb_resample', dict(action='store_true', default=False,
                               help='with --reverb_rirs: convert responses that are not 16 kHz to '
                                    '16 kHz on the GPU when they are read; without it their rate '
                                    'is ignored')),
    ('--reverb_synth', dict(type=int, default=0, metavar='N',
                            help='with --pcm_shard: N room impulse responses of shoebox rooms are '
                                 'synthesised on the GPU by the image-source method when training '
                                 'starts (the same on every rank, from --seed) and used like the '
                                 'responses of --reverb_rirs, after them when both are given; no '
                                 'measured response is needed')),
    ('--reverb_rt60', dict(type=float, nargs=2, default=list(REVERB_RT60), metavar=('LO', 'HI'),
                           help='with --reverb_synth: the nominal reverberation time of a room is '
                                'drawn uniformly in LO .. HI seconds (Sabine; the synthesised '
                                'response decays 1.2 to 1.4 times more slowly)')),
    ('--reverb_room_min', dict(type=float, nargs=3, default=list(REVERB_ROOM_MIN),
                               metavar=('X', 'Y', 'Z'),
                               help='with --reverb_synth: the smallest room in metres')),
    ('--reverb_room_max', dict(type=float, nargs=3, default=list(REVERB_ROOM_MAX),
                               metavar=('X', 'Y', 'Z'),
                               help='with --reverb_synth: the largest room in metres')),
    ('--distort', dict(type=str, nargs='+', default=None, choices=list(DISTORT_KINDS),
                       metavar='KIND',
                       help='with --pcm_shard: the signal-level distortions (clip chop bandlimit) '
                            'applied on the GPU, one per selected item drawn uniformly among '
                            'those listed, after any reverberation and before any noise is '
                            'mixed; \'_clip\' / \'_chop\' / \'_bandlimit\' is appended to the '
                            'utterance name')),
    ('--distort_prob', dict(type=float, default=1.0,
                            help='probability that an item is distorted')),
    ('--clip_factors', dict(type=float, nargs='+', default=list(CLIP_FACTORS),
                            help='with --distort clip: clipping thresholds as fractions of the '
                                 'item\'s peak, in (0, 1], drawn uniformly per item')),
    ('--chop_max', dict(type=int, default=CHOP_MAX,
                        help='with --distort chop: the most chunks removed from an item (1 .. 8)')),
    ('--chop_durs', dict(type=float, nargs=2, default=list(CHOP_DURS), metavar=('LO', 'HI'),
                         help='with --distort chop: a chunk lasts LO .. HI seconds')),
    ('--bandlimit_cutoffs', dict(type=float, nargs='+', default=list(BANDLIMIT_CUTOFFS),
                                 help='with --distort bandlimit: low-pass cutoffs in Hz, drawn '
                                      'uniformly per item')),
    ('--whisper', dict(action='store_true', default=False,
                       help='with --pcm_shard: each selected item is turned into pseudo-whisper on '
                            'the GPU (noise-excited LPC resynthesis: the spectral envelope and the '
                            'energy of every frame stay, the voiced excitation becomes noise) '
                            'before any reverberation, distortion or noise; the clean slice stays '
                            'the target and \'_whisper\' is appended to the utterance name')),
    ('--whisper_prob', dict(type=float, default=1.0,
                            help='probability that an item is whispered')),
    ('--whisper_tilts', dict(type=float, nargs='+', default=list(WHISPER_TILTS),
                             help='with --whisper: spectral tilts of the noise excitation in [0, 1) '
                                  '(0: white; 0.9: nearly +6 dB per octave), drawn uniformly per '
                                  'item')),
    ('--whisper_lag_hz', dict(type=float, default=WHISPER_LAG_HZ,
                              help='with --whisper: width in Hz of the lag window that smooths the '
                                   'spectral envelope (0 .. 1000)')),
]


def _needs_pcm_shard(opts, flag, does):
    if getattr(opts, 'pcm_shard', None) is None or getattr(opts, 'synthetic', 0) > 0:
        raise SystemExit('{} {} the batches of a pcm16 shard on the GPU: it is valid only together '
                         'with --pcm_shard PREFIX'.format(flag, does))


def _prob_in_range(flag, prob):
    if not 0.0 <= prob <= 1.0:
        raise SystemExit('{} must lie in 0 .. 1, got {}'.format(flag, prob))


def _refuse_orphans(orphans):
    """orphans: (moved, message) pairs, `moved` true when a sub-flag was given without the flag it
    belongs to; the first such pair exits with its message."""
    for moved, message in orphans:
        if moved:
            raise SystemExit(message)


def _stage_on(opts, on, flag, does, orphans=()):
    """What the check_*_flags of the loader's stages share.  A stage that is off tolerates none of
    its sub-flags (`orphans`) and yields False; one that is on needs --pcm_shard."""
    if not on:
        _refuse_orphans(orphans)
        return False
    _needs_pcm_shard(opts, flag, does)
    return True


def check_additive_flags(opts):
    """The --additive_* flags go together with --pcm_shard; anything else exits with a message."""
    noises = getattr(opts, 'additive_noises', None)
    snrs = list(getattr(opts, 'additive_snrs', [0, 5, 10]))
    prob = getattr(opts, 'additive_prob', 1.0)
    if not _stage_on(opts, noises is not None, '--additive_noises', 'mixes noise into', (
            (snrs != [0, 5, 10] or prob != 1.0,
             '--additive_snrs / --additive_prob need --additive_noises DIR'),
            (getattr(opts, 'additive_resample', False),
             '--additive_resample needs --additive_noises DIR'))):
        return False
    _prob_in_range('--additive_prob', prob)
    if len(snrs) == 0:
        raise SystemExit('--additive_snrs needs at least one level')
    return True


def check_reverb_flags(opts):
    """The --reverb_* flags go together with --pcm_shard; anything else exits with a message."""
    rirs = getattr(opts, 'reverb_rirs', None)
    prob = getattr(opts, 'reverb_prob', 1.0)
    max_taps = getattr(opts, 'reverb_max_taps', 16384)
    synth = getattr(opts, 'reverb_synth', 0)
    rt60 = list(getattr(opts, 'reverb_rt60', REVERB_RT60))
    room_min = list(getattr(opts, 'reverb_room_min', REVERB_ROOM_MIN))
    room_max = list(getattr(opts, 'reverb_room_max', REVERB_ROOM_MAX))
    if synth < 0:
        raise SystemExit('--reverb_synth must not be negative, got {}'.format(synth))
    _refuse_orphans(((synth == 0 and (rt60 != list(REVERB_RT60) or room_min != list(REVERB_ROOM_MIN)
                                      or room_max != list(REVERB_ROOM_MAX)),
                      '--reverb_rt60 / --reverb_room_min / --reverb_room_max need '
                      '--reverb_synth N'),))
    if synth > 0 and rirs is None:
        if getattr(opts, 'reverb_resample', False):
            raise SystemExit('--reverb_resample needs --reverb_rirs DIR')
        _needs_pcm_shard(opts, '--reverb_synth', 'reverberates')
    elif not _stage_on(opts, rirs is not None, '--reverb_rirs', 'reverberates', (
            (prob != 1.0 or max_taps != 16384,
             '--reverb_prob / --reverb_max_taps need --reverb_rirs DIR'),
            (getattr(opts, 'reverb_resample', False),
             '--reverb_resample needs --reverb_rirs DIR'))):
        return False
    _prob_in_range('--reverb_prob', prob)
    if max_taps < 1:
        raise SystemExit('--reverb_max_taps must be positive, got {}'.format(max_taps))
    if synth > 0:
        if not 0.0 < rt60[0] <= rt60[1]:
            raise SystemExit('--reverb_rt60 needs 0 < LO <= HI, got {}'.format(rt60))
        if not all(REVERB_ROOM_SMALLEST <= a <= b <= 50.0 for a, b in zip(room_min, room_max)):
            raise SystemExit('--reverb_room_min / --reverb_room_max need {} <= min <= max <= 50 '
                             'metres per side, got {} and {}'.format(REVERB_ROOM_SMALLEST,
                                                                     room_min, room_max))
    return True


def check_distort_flags(opts):
    """The --distort flags go together with --pcm_shard, and every sub-flag with its kind; anything
    else exits with a message.  Host arithmetic only: nothing here touches a device."""
    import math
    kinds = getattr(opts, 'distort', None)
    prob = getattr(opts, 'distort_prob', 1.0)
    factors = list(getattr(opts, 'clip_factors', CLIP_FACTORS))
    chop_max = getattr(opts, 'chop_max', CHOP_MAX)
    durs = list(getattr(opts, 'chop_durs', CHOP_DURS))
    cutoffs = list(getattr(opts, 'bandlimit_cutoffs', BANDLIMIT_CUTOFFS))
    kinds = [] if kinds is None else list(kinds)
    _refuse_orphans((      # a kind's sub-flags are orphans also when another kind is on
        (not kinds and prob != 1.0, '--distort_prob needs --distort KIND [KIND ...]'),
        ('clip' not in kinds and factors != list(CLIP_FACTORS),
         '--clip_factors needs --distort clip'),
        ('chop' not in kinds and (chop_max != CHOP_MAX or durs != list(CHOP_DURS)),
         '--chop_max / --chop_durs need --distort chop'),
        ('bandlimit' not in kinds and cutoffs != list(BANDLIMIT_CUTOFFS),
         '--bandlimit_cutoffs needs --distort bandlimit')))
    if not _stage_on(opts, bool(kinds), '--distort', 'distorts'):
        return False
    if len(set(kinds)) != len(kinds):
        raise SystemExit('--distort names a kind twice: {}'.format(' '.join(kinds)))
    _prob_in_range('--distort_prob', prob)
    if 'clip' in kinds and (len(factors) == 0 or not all(0.0 < f <= 1.0 for f in factors)):
        raise SystemExit('--clip_factors must lie in (0, 1], got {}'.format(factors))
    if 'chop' in kinds:
        if not 1 <= chop_max <= 8:
            raise SystemExit('--chop_max must lie in 1 .. 8, got {}'.format(chop_max))
        if not 0.0 < durs[0] <= durs[1] or round(durs[0] * DISTORT_SRATE) < 1:
            raise SystemExit('--chop_durs needs 0 < LO <= HI seconds and at least one sample, got '
                             '{}'.format(durs))
    if 'bandlimit' in kinds:
        if len(cutoffs) == 0 or not all(0.0 < fc < DISTORT_SRATE / 2.0 for fc in cutoffs):
            raise SystemExit('--bandlimit_cutoffs must lie above 0 and below {} Hz (half the sample '
                             'rate), got {}'.format(DISTORT_SRATE // 2, cutoffs))
        for fc in cutoffs:
            K = int(math.ceil(DISTORT_ZEROS * DISTORT_SRATE / (2.0 * fc)))
            if K > DISTORT_MAX_K:
                raise SystemExit('--bandlimit_cutoffs: {} Hz needs K = {} taps a side, more than '
                                 '{}'.format(fc, K, DISTORT_MAX_K))
    return True


def check_whisper_flags(opts):
    """The --whisper flags go together with --pcm_shard, and the sub-flags with --whisper; anything
    else exits with a message.  Host arithmetic only: nothing here touches a device."""
    prob = getattr(opts, 'whisper_prob', 1.0)
    tilts = list(getattr(opts, 'whisper_tilts', WHISPER_TILTS))
    lag_hz = getattr(opts, 'whisper_lag_hz', WHISPER_LAG_HZ)
    if not _stage_on(opts, bool(getattr(opts, 'whisper', False)), '--whisper', 'whispers', (
            (prob != 1.0 or tilts != list(WHISPER_TILTS) or lag_hz != WHISPER_LAG_HZ,
             '--whisper_prob / --whisper_tilts / --whisper_lag_hz need --whisper'),)):
        return False
    _prob_in_range('--whisper_prob', prob)
    if len(tilts) == 0 or not all(0.0 <= t < 1.0 for t in tilts):
        raise SystemExit('--whisper_tilts must lie in [0, 1), got {}'.format(tilts))
    if not 0.0 <= lag_hz <= WHISPER_MAX_LAG_HZ:
        raise SystemExit('--whisper_lag_hz must lie in 0 .. {} Hz, got {}'.format(
            int(WHISPER_MAX_LAG_HZ), lag_hz))
    return True


def build_parser():
    p = argparse.ArgumentParser(description=__doc__,
                                formatter_class=argparse.RawDescriptionHelpFormatter)
    for flag, kw in FLAGS:
        p.add_argument(flag, **kw)
    return p


def main(opts):
    use_additive = check_additive_flags(opts)
    use_reverb = check_reverb_flags(opts)
    use_distort = check_distort_flags(opts)
    use_whisper = check_whisper_flags(opts)
    if getattr(opts, 'sync_bn', False):
        os.environ['SEGAN_SYNC_BN'] = '1'
    rank, world, local = sdist.init_from_env()
    use_cuda = torch.cuda.is_available() and not opts.no_cuda
    if not use_cuda:
        raise SystemExit('segan_pytorch_amd trains only on an MI355X (HIP) device: no GPU is '
                         'visible (and there is no CPU fallback)')
    device = torch.device('cuda', local if world > 1 else 0)
    torch.cuda.set_device(device)
    opts.cuda = True
    random.seed(opts.seed)
    np.random.seed(opts.seed)
    torch.manual_seed(opts.seed)
    torch.cuda.manual_seed_all(opts.seed)
    if opts.aewsegan:
        raise NotImplementedError('AEWSEGAN is broken in the reference (model.py:823) and is '
                                  'not implemented')
    segan = (WSEGAN if opts.wsegan else SEGAN)(opts)
    from segan_pytorch_amd import ops as _sops
    if getattr(opts, 'precision', None):
        _sops.set_precision(opts.precision)
    if _sops.get_precision() == 'bf16' and not getattr(opts, 'host_z', False):
        opts.device_z = True
    if getattr(opts, 'device_z', False):
        segan.G.z_generator = torch.Generator(device=device).manual_seed(opts.seed + rank)
    opts.prefetch_z = not getattr(opts, 'no_prefetch_z', False)
    if getattr(opts, 'deterministic', False):
        from segan_pytorch_amd import ops as _ops
        _ops.set_deterministic(True)
    segan.to(device)
    print('Total model parameters: ', segan.get_n_params())
    if opts.g_pretrained_ckpt is not None:
        segan.G.load_pretrained(opts.g_pretrained_ckpt, True)
    if opts.d_pretrained_ckpt is not None:
        segan.D.load_pretrained(opts.d_pretrained_ckpt, True)
    if opts.h5:
        raise NotImplementedError('--h5 datasets are not implemented')
    collate, workers, pin = collate_fn, opts.num_workers, True
    pcm_loader = False
    if opts.synthetic > 0:
        dset = SyntheticSEDataset(opts.synthetic, opts.slice_size, seed=opts.seed)
    elif opts.pcm_shard is not None:
        if opts.preemph_norm or list(opts.random_scale) != [1]:
            raise NotImplementedError('--pcm_shard supports the default pipeline only '
                                      '(no --preemph_norm, no --random_scale)')
        dset = PCMShardDataset(opts.pcm_shard)
        # whole batches gathered by worker processes; the GPU prep kernel runs in this process
        pcm_loader = True
    else:
        dset = SEDataset(opts.clean_trainset, opts.noisy_trainset, opts.preemph,
                         cache_dir=opts.cache_dir, split='train', stride=opts.data_stride,
                         slice_size=opts.slice_size, max_samples=opts.max_samples, verbose=True,
                         preemph_norm=opts.preemph_norm, random_scale=opts.random_scale)
    sampler = None
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(dset, num_replicas=world, rank=rank, shuffle=True,
                                     seed=opts.seed, drop_last=True)
    if pcm_loader:
        from segan_pytorch_amd.datasets import PCMShardLoader
        additive = None
        if use_additive:
            from segan_pytorch_amd.augment import Additive
            additive = Additive(opts.additive_noises, opts.additive_snrs,
                                target_rate=16000 if opts.additive_resample else None)
        reverb = None
        if use_reverb:
            from segan_pytorch_amd.augment import Reverb, RIRBank
            if opts.reverb_rirs is not None:
                reverb = Reverb(opts.reverb_rirs, max_taps=opts.reverb_max_taps,
                                target_rate=16000 if opts.reverb_resample else None)
            if opts.reverb_synth > 0:
                # opts.seed, not seed + rank: every rank trains on the same rooms
                bank = RIRBank.synthetic(opts.reverb_synth, opts.seed, device,
                                         max_taps=opts.reverb_max_taps, rt60=opts.reverb_rt60,
                                         room_min=opts.reverb_room_min,
                                         room_max=opts.reverb_room_max)
                if reverb is not None:    # the responses of the files come first
                    files = reverb.bank
                    merged = RIRBank(files.rirs + bank.rirs, files=files.files + bank.files,
                                     max_taps=opts.reverb_max_taps)
                    merged.rooms = bank.rooms
                    bank = merged
                reverb = Reverb(bank)
        distort = None
        if use_distort:
            from segan_pytorch_amd import augment
            make = {'clip': lambda: augment.Clip(opts.clip_factors),
                    'chop': lambda: augment.Chop(opts.chop_max, opts.chop_durs, DISTORT_SRATE),
                    'bandlimit': lambda: augment.BandLimit(opts.bandlimit_cutoffs, DISTORT_SRATE,
                                                           DISTORT_ZEROS)}
            distort = augment.Distort({k: make[k]() for k in opts.distort})
        whisper = None
        if use_whisper:
            from segan_pytorch_amd.augment import Whisper
            whisper = Whisper(opts.whisper_tilts, opts.whisper_lag_hz)
        dloader = PCMShardLoader(dset, opts.batch_size, opts.preemph, device, sampler=sampler,
                                 drop_last=(world > 1), num_workers=max(1, min(2, opts.num_workers)),
                                 additive=additive, additive_prob=opts.additive_prob,
                                 additive_seed=opts.seed + rank, reverb=reverb,
                                 reverb_prob=opts.reverb_prob,
                                 # derived from seed + rank like the additive stream, but another
                                 # stream: the same integer would make both selections draw the
                                 # same uniforms
                                 reverb_seed=[opts.seed + rank, 1],
                                 distort=distort, distort_prob=opts.distort_prob,
                                 distort_seed=[opts.seed + rank, 2],
                                 whisper=whisper, whisper_prob=opts.whisper_prob,
                                 whisper_seed=[opts.seed + rank, 3])
    else:
        dloader = DataLoader(dset, batch_size=opts.batch_size, shuffle=(sampler is None),
                             sampler=sampler, num_workers=workers, pin_memory=pin,
                             collate_fn=collate, drop_last=(world > 1))
    va_dloader = None
    if opts.clean_valset is not None:
        # reference train.py:70-91: one pass over a batch of 300 validation slices per epoch.  The
        # objective here is the segmental SNR, computed on the device (segan_ssnr); the reference's
        # COVL / PESQ terms need the external PESQ binary and are outside the accelerated path.
        va_dset = SEDataset(opts.clean_valset, opts.noisy_valset, opts.preemph,
                            cache_dir=opts.cache_dir, split='valid', stride=opts.data_stride,
                            slice_size=opts.slice_size, max_samples=opts.max_samples, verbose=True,
                            preemph_norm=opts.preemph_norm)
        va_dloader = DataLoader(va_dset, batch_size=300, shuffle=False,
                                num_workers=opts.num_workers, pin_memory=True,
                                collate_fn=collate_fn)
    # per-rank host RNG streams for z and the phase shifts
    random.seed(opts.seed + rank)
    torch.manual_seed(opts.seed + rank)
    try:
        segan.train(opts, dloader, losses.MSELoss(), opts.l1_weight, opts.l1_dec_step,
                    opts.l1_dec_epoch, opts.save_freq, va_dloader=va_dloader, device=device)
    finally:
        sdist.destroy_native()      # the library-owned RCCL communicators (SEGAN_COMM=native)


if __name__ == '__main__':
    opts = build_parser().parse_args()
    opts.bias = not opts.no_bias
    os.makedirs(opts.save_path, exist_ok=True)
    if int(os.environ.get('RANK', '0')) == 0:
        with open(os.path.join(opts.save_path, 'train.opts'), 'w') as cfg_f:
            cfg_f.write(json.dumps(vars(opts), indent=2))
        print('Parsed arguments: ', json.dumps(vars(opts), indent=2))
    main(opts)
