"""Cut a clean/noisy wav directory pair into a pre-sliced int16 shard for
`train.py --pcm_shard PREFIX` (format: segan_pytorch_amd/datasets.py:build_pcm_shard).
usage: python scripts/make_pcm_shard.py CLEAN_DIR NOISY_DIR OUT_PREFIX [--slice_size 16384] [--stride 0.5]
       [--resample [--resample_zeros 32] [--resample_beta 8.6]]
The rate in the wav headers is ignored unless --resample is given: files that are not 16 kHz are
then converted to 16 kHz int16 on the GPU before they are sliced."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from segan_pytorch_amd.datasets import build_pcm_shard
from segan_pytorch_amd.resample import TARGET_RATE, add_filter_flags

def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument('clean_dir')
    ap.add_argument('noisy_dir')
    ap.add_argument('out_prefix')
    ap.add_argument('--slice_size', type=int, default=16384)
    ap.add_argument('--stride', type=float, default=0.5)
    ap.add_argument('--max_samples', type=int, default=None)
    ap.add_argument('--resample', action='store_true', default=False,
                    help='convert wavs that are not 16 kHz to 16 kHz int16 on the GPU first')
    add_filter_flags(ap)
    return ap


if __name__ == '__main__':
    a = build_parser().parse_args()
    n = build_pcm_shard(a.clean_dir, a.noisy_dir, a.out_prefix, a.slice_size, a.stride, a.max_samples,
                        target_rate=TARGET_RATE if a.resample else None,
                        resample_zeros=a.resample_zeros, resample_beta=a.resample_beta)
    print('{} slices -> {}.pcm16 / .json'.format(n, a.out_prefix))
