"""The ``segan_src`` operand through every contraction path, bit for bit against fp64.

Every contraction (segan_conv.hip, segan_conv_bf2.hip, segan_conv_edge.hip, segan_wgrad.hip,
segan_wgrad_bf2.hip) reads its activation through a ``segan_src``: up to two channel segments, an
optional per-channel scale / shift / slope, then roll and reflect or zero padding.  The operand
selects code (``xf_mode``, ``corr2_ok``, the materialised ``lo`` of the weight gradient, its four
LO_ID x HI_ID instantiations, the identity / transform and run / per-sample paths of
``act_pack_kernel``), and the tolerance bars of the other modules (2e-2 of max|ref| in bf16) cannot
see one wrong tap among N K = 2000 - 8000.  Here the OPERAND varies over a small fixed set of
launch plans; tests/src_sweep_cases.py holds the table, the input builders and the references.

Exact leg.  Value sets: activations integers of [-8, 8]; scale of {-2, -1, 1, 2}; shift an integer
of [-4, 4]; slope of {0, 0.25, 0.5, 1, -0.5}; weights, bias, da / dy integers of [-4, 4]; the dw
pre-fill integers of [-1000, 1000].  A transformed value is a multiple of 1/4 of at most 80 units
(bf16's 8-bit significand holds it; ``fmaf(x, scale, shift)`` is exact; the gate ``v > 0`` is decided
on an exact integer in fp32 as in fp64), so every product is a multiple of 2^-2 (2^-4 where both
weight-gradient operands are transformed).  The CONDITION, computed per case in fp64 and asserted
by the unmarked CPU test below: the same contraction over absolute values (for dw: twice it plus the
pre-fill), in units of the smallest product, is below 2^24.  Then every partial sum in ANY order is
an fp32 number: summation order, stream-K cuts, atomics, blocked accumulation and the bf16
rounding cannot change a bit, the second and third bf16x3 planes are zero (which is why the
random-valued bf16x3 tests of test_gpu_kernels.py stay the check on rounding), and the assertion is
``torch.equal(got, ref_fp64.float())`` over all elements.  Outputs the wrappers allocate with
``torch.empty`` are preceded by a freed NaN block of their size; dw is pre-filled and must be
pre-fill + ref after one call and pre-fill + 2 ref after two.

Which kernel ran is part of every assertion: ``last_corr_launch()`` / ``last_wgrad_launch()`` must
name the kernel the table states for the case and precision (and the ``xf_mode`` of the operand);
the VALU edge kernels and the short-row data gradient leave no record, which must then be unchanged.
A bf16 case is either kernel 3 or listed with the fp32 kernel it falls back to, and the CPU test
checks every listed id against a restatement of the launchers' rules.  The closing test asserts
that corr kernels 1, 2, 3 were each reached with xf_mode 0, 1, 2 and weight-gradient kernels
1, 2, 3, 4 each with lo / hi plain-plain, one transformed (either), both transformed.

Random leg (cases marked ``rand``; fp32 and bf16x3): N(0, 1) activations, |scale| of [0.5, 1.5],
N(0, 1) shifts, slopes of [-0.1, 0.3], every gate argument at least 1e-3 from zero on its own side
(asserted on the fp64 reference side); bars 3e-5 (fp32) and 5e-5 (bf16x3) of max|ref|, as in
test_gpu_kernels.py.  Measured maxima of max|err| / max|ref| on an MI355X (fp32 / bf16x3): conv1d_fwd
9.4e-7 / 8.5e-7, deconv1d_fwd 5.0e-7 / 4.2e-7, wgrad 6.4e-7 / 3.6e-7, conv1d_dgrad 6.8e-7 / 7.6e-7,
conv1d_dgrad_short 1.4e-7, deconv1d_dgrad 4.5e-7 / 4.1e-7.  The bars are not derived from these.

Base-pointer alignment (include/segan_hip.h, segan_src): 4 bytes for the input of conv1d_fwd /
deconv1d_fwd and for the weight gradient's hi in every precision — one case per path with both
segments 4 bytes past a 16-byte boundary, bit-exact; 16 bytes for the weight gradient's lo, which
every kernel reads as 16-byte vectors: segan_wgrad refuses such a pointer, asserted here without a
launch.

Size and time: 414 GPU tests (328 exact, 69 random-valued, 16 on alignment, the closing one) and 7
CPU tests.  Measured on an MI355X: 2.1 s for the whole module (pytest's total, fp64 references
included; the slowest test 0.7 s, which loads the library); the rest of the GPU suite, which is
the parent commit's, takes 408 s.
"""
import contextlib

import pytest
import torch

import src_sweep_cases as T
from segan_pytorch_amd import _lib, ops

gpu = pytest.mark.gpu
DEV = 'cuda'
BARS = {'fp32': 3e-5, 'bf16x3': 5e-5}           # of max|ref| (test_gpu_kernels.py: TOL, PREC_TOL)

SEEN_CORR = set()        # (kernel id, xf_mode)
SEEN_WGRAD = set()       # (kernel id, lo transformed, hi transformed)
WORST = {}               # random leg: (consumer, precision) -> worst max_rel


# ---------------------------------------------------------------------------------------------
# the table itself (no GPU)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', list(T.TABLES))
def test_table_is_exact_and_states_the_launchers_choice(kind):
    worst = 0.0
    for c in T.TABLES[kind]:
        worst = max(worst, T.check_exact(c))
        assert set(c.kern) <= set(T.PRECISIONS) and 'fp32' in c.kern, c.name
        for prec, want in c.kern.items():
            assert T.plan(c, prec) == want, (c.name, prec, T.plan(c, prec), want)
    print('{}: largest |contraction| = {:.3g} units (bound 2^24 = {:.3g})'.format(kind, worst, 2.0 ** 24))


def _seg_kind(seg):
    return 'single' if seg[1] == 0 else ('equal' if seg[0] == seg[1] else 'unequal')


def _roll_kind(roll, L):
    return 'zero' if roll == 0 else ('near L' if abs(roll) > L - 8 else ('positive' if roll > 0 else 'negative'))


def test_table_crosses_every_axis_on_every_consumer():
    subsets = {''.join(x for x, on in zip('chl', (a, b, c)) if on)
               for a in (0, 1) for b in (0, 1) for c in (0, 1)}
    segs, rolls = {'single', 'equal', 'unequal'}, {'zero', 'positive', 'negative', 'near L'}
    F, Dc, W = T.CONV_FWD, T.DECONV_FWD, T.WGRAD
    operands = {'conv_fwd': [(c.seg, c.xf) for c in F], 'deconv_fwd': [(c.seg, c.xf) for c in Dc],
                'wgrad hi': [c.hi for c in W], 'wgrad lo': [c.lo for c in W]}
    for who, ops_ in operands.items():
        assert {xf for _, xf in ops_} == subsets, who
        assert {_seg_kind(s) for s, _ in ops_} == segs, who
    by_kernel = {'wgrad kernel {}'.format(k): [c for c in W if c.kern['fp32'] == k] for k in (1, 2, 4)}
    for who, cs in [('conv_fwd', F), ('wgrad hi', W)] + list(by_kernel.items()):
        assert {_roll_kind(c.roll, c.L) for c in cs} == rolls, who
    for who, cs in (('conv_fwd', F), ('wgrad hi', W)):
        assert any(c.mode == T.ZERO and c.padL > 0 and 'h' in (c.xf if who == 'conv_fwd' else c.hi[1])
                   for c in cs), who
        assert any(c.mode == T.REFLECT for c in cs), who
    assert {c.S for c in F} == {1, 2, 4}
    assert {p for c in F for p in c.kern} == set(T.PRECISIONS) == {p for c in Dc for p in c.kern}
    assert {p for c in W for p in c.kern} == {'fp32', 'bf16x3', 'bf16'}
    # 'blocked' is listed only where the launch record can vouch for it: corr2_kernel on the
    # stride-4 128-row tile, the one form launch_corr2_t builds with blocked accumulation
    for c in T.ALL:
        if 'blocked' in c.kern:
            rows128 = c.M > 64 if c.kind in ('conv_fwd', 'deconv_dgrad') else True
            assert c.kern['blocked'] == 2 and c.S == 4 and rows128, c.name
    # the deterministic slabs are really used (more than one split) behind a materialised lo with
    # a transformed hi on wgrad2_kernel, and on the tiled and the edge kernel
    assert any(c.want_splits and c.kern['fp32'] == 2 and c.hi[1] and (c.lo[1] or c.lo[0][1]) for c in W)
    assert all(any(c.want_splits and c.kern['fp32'] == k for c in W) for k in (1, 2, 4))
    # a packed 16-byte piece straddles the segments: C0 odd at stride 4 (F form, 2 channels per
    # piece), C0 % 8 != 0 in the T form (8 channels per piece), on the bf16 kernels
    assert any(c.S == 4 and c.seg[1] and c.seg[0] % 2 and c.kern.get('bf16') == 3 for c in F)
    assert any(c.seg[1] and c.seg[0] % 8 and c.kern.get('bf16') == 3 for c in Dc)
    assert any(c.B >= 2 for c in T.ALL) and any(c.M == 130 or c.N == 130 for c in T.ALL)


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def dev(t):
    return None if t is None else t.to(DEV)


def off4(t):
    """A device copy 4 bytes past a 16-byte boundary (the `place_unaligned` idiom of
    test_gpu_pointwise_sweep.py)."""
    if t is None:
        return None
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def to_src(s, place=dev):
    return ops.Src(place(s.t0), place(s.t1), scale=dev(s.scale), shift=dev(s.shift), slope=dev(s.slope))


def poison(*shape):
    """Best effort: leave a freed NaN block of the output's size for torch.empty to pick up."""
    n = 1
    for d in shape:
        n *= d
    t = torch.full((n,), float('nan'), device=DEV, dtype=torch.float32)
    del t


@contextlib.contextmanager
def mode(prec):
    """'fp32' | 'det' (fp32, deterministic weight gradients) | 'blocked' | 'bf16x3' | 'bf16'."""
    try:
        if prec == 'blocked':
            ops.set_accumulation('blocked')
        elif prec == 'det':
            ops.set_deterministic(True)
        elif prec != 'fp32':
            ops.set_precision(prec)
        yield
    finally:
        ops.set_precision('fp32')
        ops.set_accumulation('plain')
        ops.set_deterministic(False)


def corr_call(c, prec, xfm, fn):
    """Run fn() in `prec` and hold the launch record against the table."""
    before = ops.last_corr_launch()
    with mode(prec):
        out = fn()
    rec = ops.last_corr_launch()
    want = c.kern[prec]
    if want == T.NOREC:
        assert rec == before, (c.name, prec, 'a kernel without a launch record was expected', rec)
    else:
        assert (rec['kernel'], rec['xf_mode']) == (want, xfm), (c.name, prec, rec)
        SEEN_CORR.add((want, xfm))
    return out


def same(what, got, want64):
    """Bit equality with the fp64 reference rounded to fp32 (exact by the table's condition)."""
    want = want64.float()
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        at = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError('{}: {} of {} elements differ, first at {}: got {!r}, want {!r}'.format(
            what, int(bad.sum()), bad.numel(), at, got[at].item(), want[at].item()))


def close(what, prec, got, want64):
    ref = want64.abs().max().item()
    e = (got.detach().double().cpu() - want64).abs().max().item() / (ref if ref > 0 else 1.0)
    key = (what.split(':')[0], prec)
    WORST[key] = max(WORST.get(key, 0.0), e)
    print('{} {}: max_rel = {:.3g} (bar {:g})'.format(what, prec, e, BARS[prec]))
    assert got.shape == want64.shape and e <= BARS[prec], (what, prec, e)


def check(what, prec, exact, got, want64):
    if exact:
        same('{} {}'.format(what, prec), got, want64)
    else:
        close(what, prec, got, want64)


# ---------------------------------------------------------------------------------------------
# the consumers
# ---------------------------------------------------------------------------------------------
def run_conv_fwd(c, prec, exact=True, place=dev):
    i = T.inputs(c, exact)
    src, w, b = to_src(i.src, place), dev(i.w), dev(i.b)
    poison(c.B, c.M, c.L // c.S)
    out = corr_call(c, prec, T.xf_mode(c.xf), lambda: ops.conv1d_fwd(
        src, w, b, c.S, roll=c.roll, pad_mode=c.mode, padL=c.padL))
    check('conv_fwd: ' + c.name, prec, exact, out, i.ref)


def run_deconv_fwd(c, prec, exact=True, place=dev):
    i = T.inputs(c, exact)
    src, w, b = to_src(i.src, place), dev(i.w), dev(i.b)
    poison(c.B, c.N, c.S * c.Ls)
    out = corr_call(c, prec, T.xf_mode(c.xf), lambda: ops.deconv1d_fwd(src, w, b, c.S))
    check('deconv_fwd: ' + c.name, prec, exact, out, i.ref)


def run_wgrad(c, prec, exact=True, place=dev):
    i = T.inputs(c, exact)
    lo, hi = to_src(i.lo), to_src(i.hi, place)
    dw = dev(i.prefill).clone()
    args = (c.K, c.S, c.padL, c.mode)
    with mode(prec):
        ops.wgrad(lo, hi, dw, *args, roll=c.roll)
        rec = ops.last_wgrad_launch()
        once = dw.clone()
        ops.wgrad(lo, hi, dw, *args, roll=c.roll)
    want = c.kern['fp32' if prec == 'det' else prec]
    assert rec['kernel'] == want, (c.name, prec, rec)
    SEEN_WGRAD.add((want, bool(c.lo[1]), bool(c.hi[1])))
    if prec == 'det' and c.want_splits:
        # the partial tiles really went through the slabs (behind a materialised lo, if any)
        assert rec['splits'] > 1, (c.name, rec)
    pre = i.prefill.double()
    check('wgrad: ' + c.name, prec if prec != 'det' else 'fp32', exact, once, pre + i.ref)
    check('wgrad twice: ' + c.name, prec if prec != 'det' else 'fp32', exact, dw, pre + 2 * i.ref)


def run_conv_dgrad(c, prec, exact=True):
    i = T.inputs(c, exact)
    da, w = dev(i.da), dev(i.w)
    poison(c.B, c.N, c.L)
    dx = corr_call(c, prec, 0, lambda: ops.conv1d_dgrad(da, w, c.L, c.S, roll=c.roll, padL=c.padL))
    check('conv_dgrad: ' + c.name, prec, exact, dx, i.ref)


def run_dgrad_short(c, prec, exact=True):
    i = T.inputs(c, exact)
    da, w = dev(i.da), dev(i.w)
    poison(c.B, c.N, c.L)
    dx = corr_call(c, prec, 0, lambda: ops.conv1d_dgrad_short(da, w, c.L, c.S, roll=c.roll, padL=c.padL))
    check('dgrad_short: ' + c.name, prec, exact, dx, i.ref)


def run_deconv_dgrad(c, prec, exact=True):
    i = T.inputs(c, exact)
    dy, w = dev(i.dy), dev(i.w)
    poison(c.B, c.M0, c.Ls)
    poison(c.B, c.M - c.M0, c.Ls)
    dx0, dx1 = corr_call(c, prec, 0, lambda: ops.deconv1d_dgrad(dy, w, c.S, c.M0, need0=c.need0))
    if c.M0 > 0 and c.need0:
        check('deconv_dgrad dx0: ' + c.name, prec, exact, dx0, i.ref[:, :c.M0])
    else:
        assert dx0 is None
    check('deconv_dgrad dx1: ' + c.name, prec, exact, dx1, i.ref[:, c.M0:])


RUN = {'conv_fwd': run_conv_fwd, 'deconv_fwd': run_deconv_fwd, 'wgrad': run_wgrad,
       'conv_dgrad': run_conv_dgrad, 'dgrad_short': run_dgrad_short, 'deconv_dgrad': run_deconv_dgrad}


def _pairs(cases):
    p = T.by_prec(cases)
    return dict(argvalues=p, ids=T.pair_ids(p))


@gpu
@pytest.mark.parametrize('c,prec', **_pairs(T.CONV_FWD))
def test_conv1d_fwd_exact(c, prec):
    run_conv_fwd(c, prec)


@gpu
@pytest.mark.parametrize('c,prec', **_pairs(T.DECONV_FWD))
def test_deconv1d_fwd_exact(c, prec):
    run_deconv_fwd(c, prec)


WGRAD_PAIRS = [(c, p) for c in T.WGRAD for p in ('fp32', 'det', 'bf16x3', 'bf16')]


@gpu
@pytest.mark.parametrize('c,prec', WGRAD_PAIRS, ids=T.pair_ids(WGRAD_PAIRS))
def test_wgrad_exact(c, prec):
    run_wgrad(c, prec)


@gpu
@pytest.mark.parametrize('c,prec', **_pairs(T.CONV_DGRAD + T.DGRAD_SHORT))
def test_conv1d_dgrad_exact(c, prec):
    RUN[c.kind](c, prec)


@gpu
@pytest.mark.parametrize('c,prec', **_pairs(T.DECONV_DGRAD))
def test_deconv1d_dgrad_exact(c, prec):
    run_deconv_dgrad(c, prec)


# ---------------------------------------------------------------------------------------------
# random-valued leg: fmaf rounding and non-trivial second / third bf16x3 planes
# ---------------------------------------------------------------------------------------------
RANDOM = [(c, p) for c in T.ALL if c.rand for p in ('fp32', 'bf16x3') if p in c.kern]


@gpu
@pytest.mark.parametrize('c,prec', RANDOM, ids=T.pair_ids(RANDOM))
def test_random_valued_leg(c, prec):
    RUN[c.kind](c, prec, exact=False)


# ---------------------------------------------------------------------------------------------
# base-pointer alignment
# ---------------------------------------------------------------------------------------------
def _first(cases, prec, kernel):
    return next(c for c in cases if c.kern.get(prec) == kernel and (c.kind == 'wgrad' or c.seg[1]))


UNALIGNED = [
    # conv1d_fwd: corr_kernel, corr2_kernel, the edge kernel, act_pack_kernel (F form)
    (_first(T.CONV_FWD, 'fp32', 1), 'fp32'), (_first(T.CONV_FWD, 'fp32', 2), 'fp32'),
    (_first(T.CONV_FWD, 'fp32', T.NOREC), 'fp32'), (_first(T.CONV_FWD, 'bf16', 3), 'bf16'),
    # deconv1d_fwd: the same, T form
    (_first(T.DECONV_FWD, 'fp32', 1), 'fp32'), (_first(T.DECONV_FWD, 'fp32', 2), 'fp32'),
    (_first(T.DECONV_FWD, 'fp32', T.NOREC), 'fp32'), (_first(T.DECONV_FWD, 'bf16', 3), 'bf16'),
    # wgrad's hi: wgrad_kernel, wgrad2_kernel, wgrad_edge_kernel, wgrad_pack_hi_kernel
    (next(c for c in T.WGRAD if c.kern['fp32'] == 1 and c.hi[0][1]), 'fp32'),
    (next(c for c in T.WGRAD if c.kern['fp32'] == 2 and c.hi[0][1]), 'fp32'),
    (next(c for c in T.WGRAD if c.kern['fp32'] == 4 and c.hi[0][1]), 'fp32'),
    (next(c for c in T.WGRAD if c.kern['bf16'] == 3 and c.hi[0][1]), 'bf16'),
]


@gpu
@pytest.mark.parametrize('c,prec', UNALIGNED, ids=T.pair_ids(UNALIGNED))
def test_segments_four_bytes_past_a_16_byte_boundary(c, prec):
    RUN[c.kind](c, prec, place=off4)


@gpu
@pytest.mark.parametrize('prec', ['fp32', 'det', 'bf16x3', 'bf16'])
def test_wgrad_refuses_a_lo_that_is_not_16_byte_aligned(prec):
    """Every weight-gradient kernel reads lo as 16-byte vectors: the entry point refuses the pointer
    (SEGAN_EINVAL and a message) before anything is launched, and dw stays as it was."""
    c = next(c for c in T.WGRAD if c.lo[0][1])
    i = T.inputs(c, True)
    dw = dev(i.prefill).clone()
    for which in ('t0', 't1'):
        lo = to_src(i.lo, lambda t, w=which: off4(t) if t is getattr(i.lo, w) else dev(t))
        with mode(prec):
            with pytest.raises(RuntimeError, match='16-byte aligned'):
                ops.wgrad(lo, to_src(i.hi), dw, c.K, c.S, c.padL, c.mode, roll=c.roll)
        assert '16-byte aligned' in _lib.load().segan_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), i.prefill)


# ---------------------------------------------------------------------------------------------
# closing: what the module reached
# ---------------------------------------------------------------------------------------------
@gpu
def test_every_kernel_and_transform_cell_was_reached():
    if not SEEN_CORR and not SEEN_WGRAD:
        pytest.skip('the sweep did not run in this session')
    print('corr (kernel, xf_mode):', sorted(SEEN_CORR))
    print('wgrad (kernel, lo transformed, hi transformed):', sorted(SEEN_WGRAD))
    print('random leg, worst max_rel:', {k: float('{:.3g}'.format(v)) for k, v in sorted(WORST.items())})
    assert SEEN_CORR >= {(k, x) for k in (1, 2, 3) for x in (0, 1, 2)}, sorted(SEEN_CORR)
    assert SEEN_WGRAD >= {(k, lo, hi) for k in (1, 2, 3, 4) for lo in (False, True)
                          for hi in (False, True)}, sorted(SEEN_WGRAD)
