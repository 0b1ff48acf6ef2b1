"""TEST-ONLY host side of tests/test_gpu_src_sweep.py: the case table, the input builders, the fp64
references and the exactness condition.  Nothing here touches a GPU.

A case names one call of one consumer of a ``segan_src`` (or of a data gradient) and, per precision
it lists, the kernel the launchers must pick for it (``kern``):

    1 corr_kernel / wgrad_kernel      2 corr2_kernel / wgrad2_kernel
    3 corr_bf2_kernel / wgrad_bf2_kernel      4 wgrad_edge_kernel
    NOREC (0): a kernel that leaves no launch record — the 1-2 channel VALU kernels of
    segan_conv_edge.hip and conv_dgrad_short_kernel; the record must then be unchanged.

A 'bf16' / 'bf16x3' entry other than 3 is a DECLINED case: the bf16 kernels refuse the geometry
(or ops.* never offers it to them) and the value is the fp32 kernel the call falls back to.
``plan_*`` restate the launchers' decisions (corr2_ok, launch_corr_f, launch_corr_tt,
segan_corr_bf2_f / _t, launch_wgrad_fp32, launch_wbf2) so that the hand-written ids of the table are
checked against them on a machine without a GPU.

Transform subsets are spelled with the letters c (scale), h (shift), l (slope).
"""
import types
import zlib

import torch
import torch.nn.functional as Fn

import emu_ops as E
from segan_pytorch_amd import layout

REFLECT, ZERO = layout.PAD_REFLECT, layout.PAD_ZERO
NOREC = 0
GATE = 1e-3
PRECISIONS = ('fp32', 'blocked', 'bf16x3', 'bf16')

# the exact leg's value sets (module docstring of test_gpu_src_sweep.py)
ACT_MAX, W_MAX, SHIFT_MAX = 8, 4, 4
SCALES = (-2.0, -1.0, 1.0, 2.0)
SLOPES = (0.0, 0.25, 0.5, 1.0, -0.5)


def ns(**kw):
    return types.SimpleNamespace(**kw)


def xf_mode(xf):
    """CorrArgs.xf_mode of a transform subset: 2 with a shift, 1 with scale / slope only, 0 none."""
    return 2 if 'h' in xf else (1 if xf else 0)


# ---------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------
def _kern(fp32, bf16x3=None, bf16=None, blocked=None):
    k = {'fp32': fp32}
    if blocked is not None:
        k['blocked'] = blocked
    if bf16x3 is not None:
        k['bf16x3'] = bf16x3
    if bf16 is not None:
        k['bf16'] = bf16
    return k


def F(name, B, seg, xf, M, L, S, kern, K=31, roll=0, mode=REFLECT, padL=None, rand=False):
    """conv1d_fwd: src [B, seg, L] -> [B, M, L / S]."""
    if padL is None:
        padL = layout.conv_pad(K, S)[0]
    return ns(kind='conv_fwd', name=name, B=B, seg=seg, xf=xf, M=M, N=sum(seg), L=L, S=S, K=K,
              roll=roll, mode=mode, padL=padL, kern=kern, rand=rand)


def D(name, B, seg, xf, N, Ls, S, kern, K=31, rand=False):
    """deconv1d_fwd: src [B, seg, Ls] -> [B, N, S * Ls]."""
    return ns(kind='deconv_fwd', name=name, B=B, seg=seg, xf=xf, M=sum(seg), N=N, Ls=Ls, S=S, K=K,
              kern=kern, rand=rand)


def W(name, B, lo, hi, Ls, S, kern, K=31, mode=REFLECT, padL=None, roll=0, want_splits=False,
      rand=False):
    """wgrad: lo = (segments, transform) [B, M, Ls], hi = (segments, transform) [B, N, S * Ls]."""
    if padL is None:
        padL = layout.conv_pad(K, S)[0] if mode == REFLECT else layout.deconv_pad(K, S)
    return ns(kind='wgrad', name=name, B=B, lo=lo, hi=hi, M=sum(lo[0]), N=sum(hi[0]), Ls=Ls, L=S * Ls,
              S=S, K=K, mode=mode, padL=padL, roll=roll, kern=kern, want_splits=want_splits, rand=rand)


def G(name, B, N, M, L, S, kern, K=31, roll=0, rand=False):
    """conv1d_dgrad: da [B, M, L / S] -> dx [B, N, L]."""
    return ns(kind='conv_dgrad', name=name, B=B, N=N, M=M, L=L, S=S, K=K, roll=roll,
              padL=layout.conv_pad(K, S)[0], kern=kern, rand=rand)


def H(name, B, N, M, L, S, K=31, roll=0, rand=False):
    """conv1d_dgrad_short (fp32 only, no launch record)."""
    return ns(kind='dgrad_short', name=name, B=B, N=N, M=M, L=L, S=S, K=K, roll=roll,
              padL=layout.conv_pad(K, S)[0], kern=_kern(NOREC), rand=rand)


def X(name, B, M, M0, N, Ls, S, kern, K=31, need0=True, rand=False):
    """deconv1d_dgrad: dy [B, N, S * Ls] -> (dx0 [B, M0, Ls], dx1 [B, M - M0, Ls])."""
    return ns(kind='deconv_dgrad', name=name, B=B, M=M, M0=M0, N=N, Ls=Ls, S=S, K=K, need0=need0,
              kern=kern, rand=rand)


CONV_FWD = [
    # stride 4.  Tcols = L / 4 columns per sample, 128-column tiles
    F('s4_5|3_chl', 3, (5, 3), 'chl', 20, 256, 4, _kern(1, 1, 1), roll=-2, rand=True),
    F('s4_24|8_cl', 2, (24, 8), 'cl', 72, 512, 4, _kern(2, 3, 3, blocked=2), roll=3, rand=True),
    F('s4_7|9_h_130', 2, (7, 9), 'h', 130, 256, 4, _kern(1, 3, 3), roll=250, rand=True),
    F('s4_12_id', 1, (12, 0), '', 40, 1024, 4, _kern(2, 2, 2)),
    F('s4_8|8_c', 3, (8, 8), 'c', 66, 128, 4, _kern(2, 3, 3, blocked=2), roll=1),
    F('s4_1|6_l', 3, (1, 6), 'l', 24, 128, 4, _kern(1, 1, 1), rand=True),
    F('s4_16_id_128', 2, (16, 0), '', 128, 256, 4, _kern(2, 3, 3, blocked=2), rand=True),
    F('s4_3|5_id', 2, (3, 5), '', 16, 256, 4, _kern(1, 1, 1), roll=-1),
    F('s4_5|4_hl_k32', 2, (5, 4), 'hl', 20, 64, 4, _kern(1, 1, 1), K=32, roll=2),
    # the shortest rows: 16 samples per tile on corr2_kernel; a 352-position window on corr_kernel
    F('s4_4_ch_L32', 3, (4, 0), 'ch', 80, 32, 4, _kern(2, 3, 3, blocked=2), roll=-1, rand=True),
    F('s4_4_l_L16', 5, (4, 0), 'l', 8, 16, 4, _kern(1, 1, 1), roll=15),
    # zero padding: with a shift a padded zero must stay zero (corr_kernel); without, corr2_kernel
    F('s4_zero_6_hl', 2, (6, 0), 'hl', 24, 256, 4, _kern(1, 1, 1), mode=ZERO, padL=5, roll=-3, rand=True),
    F('s4_zero_4|4_cl', 2, (4, 4), 'cl', 70, 512, 4, _kern(2, 2, 2, blocked=2), mode=ZERO, padL=15),
    F('s4_zero_3|5_h', 2, (3, 5), 'h', 8, 128, 4, _kern(1, 1, 1), mode=ZERO, padL=13),
    # stride 2
    F('s2_6|10_l', 2, (6, 10), 'l', 32, 512, 2, _kern(2, 2, 2), rand=True),
    F('s2_16_ch', 3, (16, 0), 'ch', 72, 128, 2, _kern(2, 3, 3), roll=-1, rand=True),
    F('s2_3|5_hl', 3, (3, 5), 'hl', 72, 128, 2, _kern(1, 3, 3), roll=120),
    F('s2_4|4_c', 2, (4, 4), 'c', 48, 64, 2, _kern(2, 2, 2)),
    # stride 1
    F('s1_8_chl', 2, (8, 0), 'chl', 8, 64, 1, _kern(2, 2, 2), roll=2, rand=True),
    F('s1_3|5_id', 2, (3, 5), '', 70, 64, 1, _kern(1, 1, 1), roll=-3),
    # 1 - 2 input channels: the VALU edge kernels (fsmall below 1024 outputs per row, fsmall4 from there)
    F('e4_1|1_chl', 2, (1, 1), 'chl', 16, 1024, 4, _kern(NOREC, NOREC, NOREC), roll=-3, rand=True),
    F('e4_2|0_cl', 2, (2, 0), 'cl', 70, 256, 4, _kern(NOREC, 3, 3), roll=2),
    F('e2_1|0_h', 3, (1, 0), 'h', 8, 512, 2, _kern(NOREC, NOREC, NOREC)),
    F('e4_1|1_hl_4096', 1, (1, 1), 'hl', 12, 4096, 4, _kern(NOREC, NOREC, NOREC), roll=4090, rand=True),
    F('e2_1|1_ch_2048', 1, (1, 1), 'ch', 70, 2048, 2, _kern(NOREC, 3, 3), roll=1),
    F('e4_zero_1|1_h', 2, (1, 1), 'h', 16, 256, 4, _kern(NOREC, NOREC, NOREC), mode=ZERO, padL=7),
    F('e1_2|0_l', 2, (2, 0), 'l', 5, 128, 1, _kern(NOREC, NOREC, NOREC), roll=1),
    F('e4_1|0_c', 2, (1, 0), 'c', 16, 64, 4, _kern(NOREC, NOREC, NOREC), roll=-60),
    F('e4_2|0_id', 2, (2, 0), '', 33, 128, 4, _kern(NOREC, NOREC, NOREC)),
]

DECONV_FWD = [
    # zero padding always: a transform with a shift runs corr_kernel.  K = 31 at stride 4 is the
    # shift mask 8 the bf16 T form takes, K = 32 (mask 12) it declines
    D('t4_24|8_cl', 3, (24, 8), 'cl', 16, 64, 4, _kern(1, 3, 3), rand=True),
    D('t4_5|3_chl', 2, (5, 3), 'chl', 40, 128, 4, _kern(1, 3, 3), rand=True),
    D('t4_8|8_l_130', 2, (8, 8), 'l', 130, 32, 4, _kern(2, 3, 3, blocked=2), rand=True),
    D('t4_12_id', 1, (12, 0), '', 8, 256, 4, _kern(2, 3, 3, blocked=2)),
    D('t4_16_h', 3, (16, 0), 'h', 24, 64, 4, _kern(1, 3, 3)),
    D('t4_8_c_Ls8', 3, (8, 0), 'c', 8, 8, 4, _kern(2, 3, 3, blocked=2)),
    D('t4_8_ch_Ls4', 3, (8, 0), 'ch', 8, 4, 4, _kern(1, 3, 3)),
    D('t4_6|10_hl_k32', 2, (6, 10), 'hl', 12, 64, 4, _kern(1, 1, 1), K=32, rand=True),
    D('t2_16_c', 2, (16, 0), 'c', 16, 256, 2, _kern(2, 3, 3), rand=True),
    D('t2_3|5_l_k32', 2, (3, 5), 'l', 32, 128, 2, _kern(2, 2, 2), K=32),
    D('t2_4|4_ch', 3, (4, 4), 'ch', 70, 64, 2, _kern(1, 3, 3)),
    # 1 - 2 output channels: the last-layer VALU kernels (tsmall; tsmall4 from 1024 columns), no tanh
    D('v4_5|3_chl', 2, (5, 3), 'chl', 1, 64, 4, _kern(NOREC, NOREC, NOREC), rand=True),
    D('v4_4|4_l', 2, (4, 4), 'l', 2, 256, 4, _kern(NOREC, NOREC, NOREC)),
    D('v4_6_c_1024', 1, (6, 0), 'c', 1, 1024, 4, _kern(NOREC, NOREC, NOREC), rand=True),
    D('v2_3|5_h', 2, (3, 5), 'h', 1, 128, 2, _kern(NOREC, NOREC, NOREC)),
    D('v4_1|7_id', 3, (1, 7), '', 2, 32, 4, _kern(NOREC, NOREC, NOREC)),
    D('v4_2|2_hl', 2, (2, 2), 'hl', 2, 64, 4, _kern(NOREC, NOREC, NOREC)),
    D('v2_8_cl', 2, (8, 0), 'cl', 2, 64, 2, _kern(NOREC, NOREC, NOREC)),
    D('v4_3|3_ch', 2, (3, 3), 'ch', 1, 128, 4, _kern(NOREC, NOREC, NOREC)),
]

PLAIN = ''
WGRAD = [
    # wgrad2_kernel (2): more than 2 hi channels and Ls a multiple of 32, or 8 / 16
    W('w2_hi5|3_chl', 2, ((20, 0), PLAIN), ((5, 3), 'chl'), 64, 4, _kern(2, 3, 3), roll=-2, rand=True),
    W('w2_lo120|10_cl_det', 3, ((120, 10), 'cl'), ((24, 0), PLAIN), 256, 4, _kern(2, 3, 3), mode=ZERO,
      want_splits=True, rand=True),
    W('w2_both', 2, ((8, 8), 'h'), ((12, 0), 'cl'), 32, 4, _kern(2, 3, 3), roll=125, rand=True),
    W('w2_s2_hi6|10_hl', 2, ((16, 0), PLAIN), ((6, 10), 'hl'), 128, 2, _kern(2, 3, 3), roll=3),
    W('w2_s1_hi3|5_c', 2, ((8, 0), PLAIN), ((3, 5), 'c'), 64, 1, _kern(2, 2, 2), roll=-1, rand=True),
    W('w2_Ls8_lo_l', 5, ((6, 0), 'l'), ((4, 4), PLAIN), 8, 4, _kern(2, 3, 3)),
    W('w2_plain', 2, ((70, 0), PLAIN), ((9, 0), PLAIN), 16, 4, _kern(2, 3, 3), roll=1),
    # middle chunks of a sample (Ls >= 96) are staged from one linear offset: the largest rolls of
    # either sign that it takes (32 S - padL = 114; -(33 S - 31 + padL) + 1 = -114); past them, and
    # near L, the call takes wgrad_kernel (the wt_roll cases below)
    W('w2_det_both_roll114', 3, ((120, 10), 'cl'), ((10, 14), 'chl'), 256, 4, _kern(2, 3, 3), roll=114,
      want_splits=True, rand=True),
    W('w2_roll-114', 2, ((20, 0), PLAIN), ((5, 3), 'hl'), 128, 4, _kern(2, 3, 3), roll=-114),
    W('w2_zero_hi_cl', 2, ((8, 0), PLAIN), ((6, 0), 'cl'), 32, 4, _kern(2, 3, 3), mode=ZERO),
    # wgrad_kernel (1): Ls neither, or zero padding with a shifted hi (a padded zero must not become
    # shift[c]: wgrad2_kernel transforms what its out-of-range loads return); bf16 declines
    # Ls % 8 != 0, bf16x3 Ls % 4 != 0
    W('wt_zero_hi_h', 2, ((8, 0), PLAIN), ((6, 0), 'h'), 32, 4, _kern(1, 3, 3), mode=ZERO),
    W('wt_zero_lo5|3_chl_hi_ch', 2, ((5, 3), 'chl'), ((3, 5), 'ch'), 64, 4, _kern(1, 3, 3), mode=ZERO,
      padL=9),
    W('wt_lo5|3_chl', 3, ((5, 3), 'chl'), ((6, 0), PLAIN), 120, 4, _kern(1, 3, 3), mode=ZERO,
      want_splits=True, rand=True),
    W('wt_roll115', 2, ((20, 0), PLAIN), ((5, 3), 'c'), 128, 4, _kern(1, 3, 3), roll=115),
    W('wt_roll-115', 2, ((8, 8), 'l'), ((12, 0), 'h'), 128, 4, _kern(1, 3, 3), roll=-115),
    W('wt_det_both_roll509', 3, ((5, 3), 'chl'), ((3, 5), 'cl'), 128, 4, _kern(1, 3, 3), roll=509,
      want_splits=True, rand=True),
    W('wt_roll-509', 2, ((20, 0), PLAIN), ((6, 0), 'ch'), 128, 4, _kern(1, 3, 3), roll=-509),
    W('wt_plain', 2, ((8, 0), PLAIN), ((5, 0), PLAIN), 12, 4, _kern(1, 3, 1), roll=-2),
    W('wt_s2_hi1|7_ch', 2, ((20, 0), PLAIN), ((1, 7), 'ch'), 20, 2, _kern(1, 3, 1), roll=3, rand=True),
    W('wt_both_130', 3, ((130, 0), 'hl'), ((4, 4), 'h'), 24, 4, _kern(1, 3, 3), roll=-93),
    W('wt_lo3|5_c', 2, ((3, 5), 'c'), ((5, 0), PLAIN), 40, 4, _kern(1, 3, 3), mode=ZERO),
    W('wt_edge_ragged_hi1|1_h', 2, ((16, 0), PLAIN), ((1, 1), 'h'), 24, 4, _kern(1, 3, 3)),
    # wgrad_edge_kernel (4): 1 - 2 hi channels, Ls a multiple of 32
    W('we_hi1|1_chl', 2, ((16, 0), PLAIN), ((1, 1), 'chl'), 64, 4, _kern(4, 3, 3), roll=-3, rand=True),
    W('we_plain', 2, ((70, 0), PLAIN), ((1, 0), PLAIN), 32, 4, _kern(4, 3, 3)),
    W('we_lo5|3_cl', 2, ((5, 3), 'cl'), ((1, 0), PLAIN), 64, 4, _kern(4, 3, 3), mode=ZERO, rand=True),
    W('we_both', 2, ((40, 0), 'h'), ((2, 0), 'l'), 32, 4, _kern(4, 3, 3), mode=ZERO),
    W('we_zero_hi1|1_ch', 2, ((20, 0), PLAIN), ((1, 1), 'ch'), 32, 4, _kern(4, 3, 3), mode=ZERO, padL=6),
    W('we_lo_ch', 2, ((24, 0), 'ch'), ((2, 0), PLAIN), 32, 4, _kern(4, 3, 3), mode=ZERO),
    W('we_det_hi_c', 2, ((16, 0), PLAIN), ((1, 0), 'c'), 1024, 4, _kern(4, 3, 3), roll=4093,
      want_splits=True),
    W('we_s2_hi1|1_hl', 2, ((8, 0), PLAIN), ((1, 1), 'hl'), 64, 2, _kern(4, 3, 3), roll=2),
]

CONV_DGRAD = [
    G('g4_12', 2, 12, 40, 256, 4, _kern(2, 3, 3, blocked=2), roll=-3, rand=True),
    G('g4_130', 2, 130, 24, 64, 4, _kern(2, 3, 3), roll=-60),
    G('g4_k5', 2, 6, 7, 128, 4, _kern(2, 3, 3), K=5),
    G('g2_16', 2, 16, 24, 512, 2, _kern(2, 3, 3), roll=2, rand=True),
    G('g1_8', 2, 8, 8, 64, 1, _kern(2, 2, 2), roll=1),
    # fp32 routes this geometry to the short-row kernel, the bf16 modes to the T form
    G('g4_short_route', 3, 8, 16, 128, 4, _kern(NOREC, 3, 3), roll=4),
    # 1 - 2 input channels: tsmall / tsmall4
    G('g4_n1', 2, 1, 16, 1024, 4, _kern(NOREC, NOREC, NOREC), roll=5, rand=True),
    G('g4_n2', 2, 2, 20, 256, 4, _kern(NOREC, NOREC, NOREC), roll=-2),
    G('g2_n2', 2, 2, 8, 128, 2, _kern(NOREC, NOREC, NOREC), roll=127),
    G('g4_n1_4096', 1, 1, 12, 4096, 4, _kern(NOREC, NOREC, NOREC), roll=-1),
]

DGRAD_SHORT = [
    H('h4_Ls16', 5, 8, 16, 64, 4, roll=3, rand=True),
    H('h2_Ls64', 2, 4, 32, 128, 2, roll=-1),
    H('h4_Ls4', 3, 4, 16, 16, 4, roll=-15),
    H('h4_Ls8', 2, 12, 48, 32, 4),
    H('h4_Ls32', 2, 8, 16, 128, 4, roll=100),
]

DECONV_DGRAD = [
    X('x4_on', 2, 192, 128, 8, 32, 4, _kern(2, 3, 3, blocked=2), rand=True),
    X('x4_off', 2, 192, 100, 8, 32, 4, _kern(2, 3, 3, blocked=2)),
    X('x4_on_skip0', 2, 192, 128, 8, 32, 4, _kern(2, 3, 3), need0=False),
    X('x4_off_skip0', 2, 192, 100, 5, 32, 4, _kern(2, 3, 3), need0=False, rand=True),
    X('x2_small', 3, 40, 24, 6, 64, 2, _kern(2, 2, 2)),
    X('x4_k32_whole', 2, 70, 0, 5, 16, 4, _kern(2, 3, 3), K=32),
]

TABLES = {'conv_fwd': CONV_FWD, 'deconv_fwd': DECONV_FWD, 'wgrad': WGRAD, 'conv_dgrad': CONV_DGRAD,
          'dgrad_short': DGRAD_SHORT, 'deconv_dgrad': DECONV_DGRAD}
ALL = [c for t in TABLES.values() for c in t]


def ids(cases):
    return [c.name for c in cases]


def by_prec(cases, precs=PRECISIONS):
    """(case, precision) pairs of the precisions each case lists."""
    return [(c, p) for c in cases for p in precs if p in c.kern]


def pair_ids(pairs):
    return ['{}-{}'.format(c.name, p) for c, p in pairs]


# ---------------------------------------------------------------------------------------------
# the launchers' decisions, restated
# ---------------------------------------------------------------------------------------------
def samples_per_tile(Tcols, NB):
    if Tcols >= NB:
        return 1 if Tcols % NB == 0 else 2
    return NB // Tcols if NB % Tcols == 0 else (NB + Tcols - 2) // Tcols + 1


def _corr2_ok(U, H, Tcols, NB, zero, xfm, C0, C1):
    SL = 4 // (32 // U)
    if NB + samples_per_tile(Tcols, NB) * H > 64 * SL * 4:
        return False
    if zero and xfm == 2:
        return False
    if C1 > 0 and C0 != C1 and samples_per_tile(Tcols, NB) > 1:
        return False
    return True


def plan_corr_f(U, M, Tcols, zero, xfm, C0, C1):
    """launch_corr_f: 2 corr2_kernel, 1 corr_kernel."""
    H = U - 1
    if U == 16 and M <= 32 and _corr2_ok(U, H, Tcols, 256, zero, xfm, C0, C1):
        return 2
    if _corr2_ok(U, H, Tcols, 128, zero, xfm, C0, C1):
        return 2
    assert 128 + samples_per_tile(Tcols, 128) * H <= 512
    return 1


def plan_corr_t(U, H, Tcols, xfm, C0, C1):
    """launch_corr_tt (its input view is always zero padded)."""
    assert 128 + samples_per_tile(Tcols, 128) * H <= 512
    return 2 if _corr2_ok(U, H, Tcols, 128, True, xfm, C0, C1) else 1


def _bf2_window_ok(Tcols, H):
    return -(-(128 + samples_per_tile(Tcols, 128) * H) // 64) <= 6


def _t_shifts(K, S):
    pad = layout.deconv_pad(K, S)
    c = [(r + pad) // S for r in range(S)]
    return [x - min(c) for x in c]


def short_rows_ok(N, M, L, S):
    return S in (2, 4) and L % S == 0 and (L // S) in (4, 8, 16, 32, 64) and N % 4 == 0 and M % 16 == 0


def plan(c, prec):
    """The kernel id the launchers pick for case c in precision prec."""
    bf = prec in ('bf16', 'bf16x3')
    U = 32 // c.S
    if c.kind == 'conv_fwd':
        zero = c.mode == ZERO
        fp = NOREC if c.N <= 2 else plan_corr_f(U, c.M, c.L // c.S, zero, xf_mode(c.xf), *c.seg)
        if bf and not zero and c.M > 64 and U in (8, 16) and _bf2_window_ok(c.L // c.S, U - 1):
            return 3
        return fp
    if c.kind == 'deconv_fwd':
        if c.N <= 2:
            return NOREC
        sh = _t_shifts(c.K, c.S)
        H = U - 1 + max(sh)
        mask = sum(1 << r for r, s in enumerate(sh) if s)
        if bf and ((U == 8 and mask in (0, 8)) or (U == 16 and mask == 0)) and _bf2_window_ok(c.Ls, H):
            return 3
        return plan_corr_t(U, H, c.Ls, xf_mode(c.xf), *c.seg)
    if c.kind == 'conv_dgrad':
        if c.N <= 2:
            return NOREC
        padR = max(c.K - c.S - c.padL, 0)
        Tcols = (c.L + c.padL + padR - 1) // c.S + 1
        if bf and U in (8, 16) and _bf2_window_ok(Tcols, U - 1):
            return 3
        if short_rows_ok(c.N, c.M, c.L, c.S):
            return NOREC
        return plan_corr_t(U, U - 1, Tcols, 0, c.M, 0)
    if c.kind == 'dgrad_short':
        assert short_rows_ok(c.N, c.M, c.L, c.S)
        return NOREC
    if c.kind == 'deconv_dgrad':
        if bf and c.M > 64 and U in (8, 16) and _bf2_window_ok(c.Ls, U - 1):
            return 3
        return plan_corr_f(U, c.M, c.Ls, True, 0, c.N, 0)
    if c.kind == 'wgrad':
        if bf and c.S in (2, 4) and c.Ls % (8 if prec == 'bf16' else 4) == 0:
            return 3
        Cv = c.N * c.S
        shifted_zero = c.mode == ZERO and 'h' in c.hi[1]
        first, last = 32 * c.S - c.padL, c.S * (c.Ls - 32 + U - 2) + c.S - 1 - c.padL
        middle_ok = c.Ls < 96 or (first >= 0 and last < c.L and first - c.roll >= 0 and last - c.roll < c.L)
        if Cv > 64 // U and (c.Ls % 32 == 0 if c.Ls >= 32 else (c.Ls >= 8 and 32 % c.Ls == 0)) \
                and not shifted_zero and middle_ok:
            return 2
        if Cv <= 64 // U and c.N <= 2 and c.Ls % 32 == 0 and c.M <= 128 and not (c.M > 64 and c.N > 1):
            return 4
        assert c.Ls % 4 == 0
        return 1
    raise ValueError(c.kind)


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def _gen(c, leg):
    return torch.Generator().manual_seed(zlib.crc32('{}/{}/{}'.format(c.kind, c.name, leg).encode()))


def _ints(g, shape, m):
    return torch.randint(-m, m + 1, tuple(shape), generator=g).float()


def _pick(g, n, values):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=g)].float()


def _vals(g, shape, exact, m, sd=1.0):
    """Integers of [-m, m] (exact leg) or N(0, sd) (random leg)."""
    return _ints(g, shape, m) if exact else (torch.randn(tuple(shape), generator=g) * sd).float()


def cat(s):
    return s.t0 if s.t1 is None else torch.cat((s.t0, s.t1), 1)


def gate_arg(s):
    """The fp64 argument of the PReLU gate of a source."""
    v = cat(s).double()
    if s.scale is not None:
        v = v * s.scale.double().view(1, -1, 1)
    if s.shift is not None:
        v = v + s.shift.double().view(1, -1, 1)
    return v


def mat(s):
    """The materialised source in fp64 (emu_ops' transform)."""
    return E._xform(cat(s), s.scale, s.shift, s.slope)


def build_src(g, B, seg, xf, L, exact):
    """A source of `seg` = (C0, C1) channels with the vectors named in `xf` non-NULL."""
    C0, C1 = seg
    C = C0 + C1
    if exact:
        x = _ints(g, (B, C, L), ACT_MAX)
        sc, sh, sl = _pick(g, C, SCALES), _ints(g, (C,), SHIFT_MAX), _pick(g, C, SLOPES)
    else:
        x = torch.randn(B, C, L, generator=g).float()
        sc = (0.5 + torch.rand(C, generator=g)) * _pick(g, C, (-1.0, 1.0))
        sh = torch.randn(C, generator=g).float()
        sl = (torch.rand(C, generator=g) * 0.4 - 0.1).float()
    s = ns(t0=None, t1=None, scale=sc if 'c' in xf else None, shift=sh if 'h' in xf else None,
           slope=sl if 'l' in xf else None)
    if not exact and xf:
        # gate-safe: every gate argument at least GATE from zero, on its own side
        s.t0 = x
        v = gate_arg(s)
        sgn = torch.where(v >= 0, 1.0, -1.0).double()
        dv = s.scale.double().view(1, -1, 1) if s.scale is not None else 1.0
        x = torch.where(v.abs() < 2 * GATE, (x.double() + (sgn * 4 * GATE - v) / dv).float(), x)
    s.t0 = x[:, :C0].contiguous()
    s.t1 = x[:, C0:].contiguous() if C1 else None
    if not exact and xf:
        assert gate_arg(s).abs().min().item() >= GATE
    return s


def conv64(x, w, b, S, roll, mode, padL):
    """out[b, m, t] = bias[m] + sum_{n, k} w[m, n, k] pad(roll(x))[b, n, S t + k], t < L / S, in the
    dtype of its arguments; the right padding is what the last output's window reaches."""
    K, L = w.shape[2], x.shape[2]
    padR = max(0, S * (L // S - 1) + K - padL - L)
    xp = Fn.pad(torch.roll(x, roll, 2), (padL, padR), mode='reflect' if mode == REFLECT else 'constant')
    return Fn.conv1d(xp, w, b, stride=S)[:, :, :L // S]


def deconv64(x, w, b, S):
    """ConvTranspose1d(stride S, padding deconv_pad) trimmed to S * Ls samples."""
    y = Fn.conv_transpose1d(x, w, b, stride=S, padding=layout.deconv_pad(w.shape[2], S))
    return y[:, :, :S * x.shape[2]]


_CACHE = {}      # (id of the case object, exact leg) -> what inputs() returns


def _grad(fn, shape, cot):
    """The adjoint of the linear map fn at `cot`, in fp64."""
    with torch.enable_grad():
        z = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        (g,) = torch.autograd.grad(fn(z), z, cot.double())
    return g


def _build(c, exact):
    kind = c.kind
    g = _gen(c, 'exact' if exact else 'random')
    i = ns(case=c, exact=exact)
    ab = torch.abs

    if kind == 'conv_fwd':
        i.src = build_src(g, c.B, c.seg, c.xf, c.L, exact)
        i.w, i.b = _vals(g, (c.M, c.N, c.K), exact, W_MAX, 0.1), _vals(g, (c.M,), exact, W_MAX)
        f = lambda x, w, b: conv64(x, w, b, c.S, c.roll, c.mode, c.padL)
        i.ref = f(mat(i.src), i.w.double(), i.b.double())
        i.bound = f(ab(mat(i.src)), ab(i.w).double(), ab(i.b).double()).max().item()
        i.unit = 0.25
    elif kind == 'deconv_fwd':
        i.src = build_src(g, c.B, c.seg, c.xf, c.Ls, exact)
        i.w, i.b = _vals(g, (c.M, c.N, c.K), exact, W_MAX, 0.1), _vals(g, (c.N,), exact, W_MAX)
        i.ref = deconv64(mat(i.src), i.w.double(), i.b.double(), c.S)
        i.bound = deconv64(ab(mat(i.src)), ab(i.w).double(), ab(i.b).double(), c.S).max().item()
        i.unit = 0.25
    elif kind == 'wgrad':
        i.lo = build_src(g, c.B, c.lo[0], c.lo[1], c.Ls, exact)
        i.hi = build_src(g, c.B, c.hi[0], c.hi[1], c.L, exact)
        if exact:
            # a weight gradient contracts an activation with a gradient (da / dy: integers of
            # [-4, 4]): the plain operand beside a transformed one, lo where both are plain
            grad = None if (c.lo[1] and c.hi[1]) else (i.hi if c.lo[1] else i.lo)
            if grad is not None:
                grad.t0 = _ints(g, grad.t0.shape, W_MAX)
                grad.t1 = _ints(g, grad.t1.shape, W_MAX) if grad.t1 is not None else None
        i.prefill = _ints(g, (c.M, c.N, c.K), 1000) if exact else torch.zeros(c.M, c.N, c.K)
        f = lambda lo, hi: _grad(
            lambda w: conv64(hi, w, None, c.S, c.roll, c.mode, c.padL), (c.M, c.N, c.K), lo)
        i.ref = f(mat(i.lo), mat(i.hi))
        i.bound = 2 * f(ab(mat(i.lo)), ab(mat(i.hi))).max().item() + 1000
        i.unit = 0.0625 if (c.lo[1] and c.hi[1]) else 0.25
    elif kind in ('conv_dgrad', 'dgrad_short'):
        i.da = _vals(g, (c.B, c.M, c.L // c.S), exact, W_MAX)
        i.w = _vals(g, (c.M, c.N, c.K), exact, W_MAX, 0.1)
        f = lambda da, w: _grad(lambda x: conv64(x, w, None, c.S, c.roll, REFLECT, c.padL),
                                (c.B, c.N, c.L), da)
        i.ref = f(i.da, i.w.double())
        i.bound = f(ab(i.da), ab(i.w).double()).max().item()
        i.unit = 1.0
    elif kind == 'deconv_dgrad':
        i.dy = _vals(g, (c.B, c.N, c.S * c.Ls), exact, W_MAX)
        i.w = _vals(g, (c.M, c.N, c.K), exact, W_MAX, 0.1)
        f = lambda dy, w: _grad(lambda x: deconv64(x, w, None, c.S), (c.B, c.M, c.Ls), dy)
        i.ref = f(i.dy, i.w.double())
        i.bound = f(ab(i.dy), ab(i.w).double()).max().item()
        i.unit = 1.0
    else:
        raise ValueError(kind)
    return i


def inputs(c, exact=True):
    """CPU inputs, the fp64 reference and the exactness bound of a case; computed once per case and
    leg (the case objects are module-level tables, here or in another sweep's module, and live as
    long as the cache) and shared: callers must leave them unchanged."""
    key = (id(c), bool(exact))
    if key not in _CACHE:
        _CACHE[key] = _build(c, bool(exact))
    return _CACHE[key]


def check_exact(c):
    """The exactness CONDITION of a case: the contraction over absolute values (plus, for dw, the
    pre-fill and the second call), in units of the smallest product, stays below 2^24 — so every
    product and every partial sum in any order is an fp32 (and bf16-operand) number.  Also: every
    operand is a multiple of 1/4 of at most 80 units (bf16's 8-bit significand)."""
    i = inputs(c, True)
    assert i.bound / i.unit < 2 ** 24, (c.name, i.bound, i.unit)
    assert torch.equal(i.ref.float().double(), i.ref), c.name
    for name in ('src', 'lo', 'hi'):
        s = getattr(i, name, None)
        if s is not None:
            m4 = mat(s) * 4
            assert torch.equal(m4, m4.round()) and m4.abs().max().item() <= 80, (c.name, name)
    for name in ('w', 'b', 'da', 'dy'):
        t = getattr(i, name, None)
        if t is not None:
            assert torch.equal(t, t.round()) and t.abs().max().item() <= W_MAX, (c.name, name)
    return i.bound / i.unit
