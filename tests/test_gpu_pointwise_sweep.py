"""Sweep of the per-channel, loss, optimizer, pooling and scan kernels against float64.

Every entry point of segan_pointwise.hip and the de-emphasis scan of segan_audio.hip runs on the
GPU and is compared with ``tests/emu_ops.py`` (the float64 restatement the CPU suite stands on, so
this module also pins emu_ops to the kernels) on CPU copies of the same fp32 inputs, or with an
inline float64 reference where emu_ops has no counterpart (de_emphasize, fill_, scale_).

What the cases are built to reach
  * the second and later trips of every capped grid-stride loop (> 2 x 1 048 576 elements);
  * the scalar path beside the float4 path (L % 4 != 0, and base pointers that are not 16-byte
    aligned: ``buf[o:o + n].view(B, C, L)``);
  * batch splits with short and empty trailing splits ((300, 8, 4096): 256 splits, 106 empty);
  * the row / thread mapping at L = 1, 2, 3, 5, 7;
  * every optional-pointer combination of include/segan_hip.h, and the accumulate-into rule of
    the d* outputs (pre-filled, called twice);
  * the slab carry of the de-emphasis scan (T around 8192).

Bars
  * elementwise outputs: max_rel <= 1e-5; the BatchNorm backward's da: 2e-5;
  * optimizers: 2e-7 absolute after 3 steps at lr = 5e-5;
  * de_emphasize: 5e-6 absolute on |y| <= 1;
  * bn_stats: mean within 5e-5 of a standard deviation, variance within 2e-4 relative;
  * per-channel and scalar SUMS: |got - want| <= gamma * 2^-24 * S with S = sum |term| from the
    float64 reference and gamma = 2 * (m + 16 + nsplit): m terms added serially by one thread,
    16 for the shuffle and LDS stages, nsplit for the final serial pass, 2 for the rounding of
    each product before it is added (``sum_tol``).  Where a term is itself a cancelling fp32
    expression, S is taken over the magnitudes before the cancellation.  A channel whose terms are
    all zero therefore has to come out exactly 0: that is what the one-hot probes use.

PReLU gates: the kernels decide ``v > 0`` in fp32 and the reference in fp64, so the inputs are built
gate-safe (every gate argument moved to |v| >= 1e-3 on its own side, asserted on the reference
side) and no element is excluded from any comparison.

Outputs are allocated inside ops.* with torch.empty; ``poison`` hands the caching allocator a
NaN-filled block of the same size just before each call so that a skipped store shows as NaN
instead of a stale, correct value.

pool_time_fwd('max') on rows that contain NaN is unspecified (AdaptiveMaxPool1d propagates the
NaN, the kernel keeps a NaN only where it is the first element a lane visits); activations on
the training path are finite and no test feeds it one.
"""
import functools
import math

import numpy as np
import pytest
import torch

import emu_ops as E
from conftest import max_rel
from segan_pytorch_amd import _lib, ops

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24          # half an ulp of fp32, relative
GATE = 1e-3

# B, C, L: every L of {1, 2, 3, 5, 7, 8, 1001, 4096}, C of {1, 5, 70, 2049}, B of {1, 2, 5, 7, 300}
SHAPES = [
    (1, 1, 1), (2, 70, 3), (5, 3, 1001), (300, 8, 4096), (300, 64, 16), (5, 2049, 8),
    (7, 5, 2), (1, 70, 5), (2, 1, 7), (7, 2049, 1), (5, 5, 8), (2, 5, 4096), (300, 5, 7),
    (300, 1, 1001),
]
BIG = (300, 8, 4096)                      # 9.8 M elements: 9 trips of a 4096 x 256 grid
UNALIGNED_SHAPES = [(5, 3, 8), (7, 5, 4096)]
ONE_HOT_SHAPES = [(300, 8, 4096), (5, 3, 1001), (300, 5, 7), (300, 64, 16), (2, 70, 3)]


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).float()


def uni(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g).float()


def dev(t):
    return None if t is None else t.to(DEV)


def place_aligned(name, t):
    return dev(t)


def place_unaligned(which, off):
    """Device copies at a base pointer `off` floats past a 16-byte boundary, for the argument
    called `which` ('all': every activation-sized argument)."""
    def place(name, t):
        if t is None or (which != 'all' and name != which):
            return dev(t)
        buf = torch.empty(t.numel() + 4, device=DEV, dtype=torch.float32)
        v = buf[off:off + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    return place


def poison(numel):
    """Best effort: leave a freed NaN block of the output's size for torch.empty to pick up."""
    t = torch.full((int(numel),), float('nan'), device=DEV, dtype=torch.float32)
    del t


def no_nan(*ts):
    for t in ts:
        if t is not None:
            assert not torch.isnan(t).any().item(), 'an output element was never stored'


def nsplit(B, C, L):
    return _lib.load().segan_bn_nsplit(B, C, L)


def chan_m(B, C, L):
    """(m, nsplit) of the per-channel reductions: one thread of a 256-thread workgroup adds
    m = ceil(rows_per_split * L / 256) terms serially."""
    ns = nsplit(B, C, L)
    per = -(-B // ns)
    return -(-per * L // 256), ns


def sum_tol(S, m, ns):
    """The derived bar of a sum: 2 * (m + 16 + ns) * 2^-24 * sum|term| (module docstring)."""
    return 2 * (m + 16 + ns) * U * S


def check_sum(what, got, want, tol):
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    want = torch.as_tensor(want).detach().double().cpu().reshape(-1)
    tol = torch.as_tensor(tol).double().reshape(-1).expand_as(want)
    err = (got - want).abs()
    live = tol > 0
    worst = (err[live] / tol[live]).max().item() if live.any() else 0.0
    print('{}: worst |err| / bar = {:.3g}; max |err| where the bar is 0 = {:.3g}'.format(
        what, worst, err[~live].max().item() if (~live).any() else 0.0))
    assert torch.isfinite(got).all(), what
    assert (err <= tol).all(), what


def check_elem(what, got, want, bar=1e-5):
    e = max_rel(got, want)
    print('{}: max_rel = {:.3g} (bar {:g})'.format(what, e, bar))
    assert got.shape == want.shape, what
    assert e <= bar, what


def nudge(x, v, dv_dx, target):
    """Move the elements of x whose fp64 gate argument v has |v| < GATE so that it becomes
    +-target on its own side; dv_dx is the (per-channel) derivative of v by x."""
    bad = v.abs() < GATE
    sign = torch.where(v >= 0, 1.0, -1.0).double()
    xn = x.double() + (sign * target - v) / dv_dx
    return torch.where(bad, xn.float(), x), bad.double().mean().item()


# ---------------------------------------------------------------------------------------------
# elementwise forwards: affine_prelu, affine_tanh, scale_mask, sum_skip
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def fwd_inputs(shape):
    B, C, L = shape
    x = rnd(B, C, L, seed=11) * 2 + 0.3
    x1 = rnd(B, C, L, seed=12)
    mask = (uni(B, C, L, seed=13) > 0.5).float() * 2.0
    scale, shift = rnd(C, seed=14) + 1.5, rnd(C, seed=15)
    slope, alpha = rnd(C, seed=16).abs() * 0.3, rnd(C, seed=17)
    return dict(x=x, x1=x1, mask=mask, scale=scale, shift=shift, slope=slope, alpha=alpha)


FWD_OPS = ('affine_prelu', 'affine_tanh', 'scale_mask', 'sum_skip')
FWD_OPTIONAL = {'affine_prelu': ('scale', 'shift', 'slope'), 'affine_tanh': ('scale', 'shift'),
                'scale_mask': ('scale',), 'sum_skip': ('slope',)}


def run_fwd(op, shape, place=place_aligned, drop=()):
    """One forward op on the GPU against emu_ops; `drop` names the optional vectors passed as
    None.  Returns the GPU output."""
    i = fwd_inputs(shape)
    p = {k: (None if k in drop else v) for k, v in i.items()}
    n = i['x'].numel()
    if op == 'affine_prelu':
        want = E.affine_prelu(p['x'], p['scale'], p['shift'], p['slope'])
        xg = place('x', p['x'])
        poison(n)
        got = ops.affine_prelu(xg, dev(p['scale']), dev(p['shift']), dev(p['slope']))
    elif op == 'affine_tanh':
        want = E.affine_tanh(p['x'], p['scale'], p['shift'])
        xg = place('x', p['x'])
        poison(n)
        got = ops.affine_tanh(xg, dev(p['scale']), dev(p['shift']))
    elif op == 'scale_mask':
        want = E.scale_mask(p['x'], p['scale'], p['mask'])
        xg, mg = place('x', p['x']), place('mask', p['mask'])
        poison(n)
        got = ops.scale_mask(xg, dev(p['scale']), mg)
    else:
        want = E.sum_skip(p['x'], p['slope'], p['x1'], p['alpha'])
        xg, x1g = place('x', p['x']), place('x1', p['x1'])
        poison(n)
        got = ops.sum_skip(xg, dev(p['slope']), x1g, dev(p['alpha']))
    no_nan(got)
    check_elem('{} {} drop={}'.format(op, shape, drop), got, want)
    return got


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('op', FWD_OPS)
def test_forward_grid(op, shape):
    run_fwd(op, shape)


@pytest.mark.parametrize('op', FWD_OPS)
def test_forward_optional_arguments(op):
    names = FWD_OPTIONAL[op]
    for mask in range(1, 2 ** len(names)):
        drop = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        for shape in ((5, 3, 1001), (5, 5, 8)):
            run_fwd(op, shape, drop=drop)


@pytest.mark.parametrize('shape', UNALIGNED_SHAPES)
@pytest.mark.parametrize('op', FWD_OPS)
def test_forward_unaligned_views_are_bit_equal(op, shape):
    base = run_fwd(op, shape)
    second = {'scale_mask': 'mask', 'sum_skip': 'x1'}.get(op)
    for off in (1, 2, 3):
        for which in ('x', second, 'all'):
            if which is None:
                continue
            got = run_fwd(op, shape, place=place_unaligned(which, off))
            assert torch.equal(got, base), (op, which, off)


def test_scale_mask_in_place():
    """include/segan_hip.h: y may alias x.  ops.scale_mask allocates y, so call the library."""
    i = fwd_inputs((5, 3, 1001))
    want = E.scale_mask(i['x'], i['scale'], i['mask'])
    xg, mg, sg = dev(i['x']).clone(), dev(i['mask']), dev(i['scale'])
    B, C, L = xg.shape
    _lib.check(_lib.load().segan_scale_mask(ops._ptr(xg), ops._ptr(sg), ops._ptr(mg), ops._ptr(xg),
                                            B, C, L, ops._stream()), 'scale_mask')
    check_elem('scale_mask in place', xg, want)


# ---------------------------------------------------------------------------------------------
# BatchNorm statistics
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def bn_inputs(shape):
    B, C, L = shape
    x = rnd(B, C, L, seed=21) * 2 + 0.3 + rnd(C, seed=22).view(1, C, 1)
    return dict(x=x, gamma=rnd(C, seed=23) + 1.5, beta=rnd(C, seed=24),
                rm=rnd(C, seed=25), rv=uni(C, seed=26) + 0.5)


def check_stats(what, shape, got, x, gamma, beta, eps, rm0=None, rv0=None, rm=None, rv=None,
                momentum=0.1):
    """(mean, rstd, scale, shift) [+ running statistics] against float64 at the bn_stats bars."""
    B, C, L = shape
    n = B * L
    mean, rstd, scale, shift = (t.double().cpu() for t in got)
    no_nan(*got)
    xd = x.double()
    mean_ref = xd.mean((0, 2))
    var_ref = xd.var((0, 2), unbiased=False)
    if n == 1:
        # one element per channel: the mean is that element and the variance exactly zero
        assert torch.equal(mean, mean_ref) and eps > 0
        check_elem(what + ' rstd', rstd, torch.full((C,), eps ** -0.5, dtype=torch.float64), 1e-6)
        var = var_ref
    else:
        var = 1.0 / rstd ** 2 - eps
        emean = ((mean - mean_ref).abs() / var_ref.sqrt()).max().item()
        evar = ((var - var_ref).abs() / var_ref).max().item()
        print('{}: mean err / sd = {:.3g} (bar 5e-5), var rel err = {:.3g} (bar 2e-4)'.format(
            what, emean, evar))
        assert emean <= 5e-5, what
        assert evar <= 2e-4, what
    # scale = gamma * rstd and shift = beta - mean * scale from the kernel's OWN mean / rstd: one
    # rounding each for the product, the fma and the fp32 rstd the kernel derived scale from
    ga = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    be = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    assert ((scale - ga * rstd).abs() <= 4 * U * (ga * rstd).abs()).all(), what
    assert ((shift - (be - mean * scale)).abs() <= 4 * U * (be.abs() + (mean * scale).abs())).all(), what
    if rm is not None:
        rm, rv = rm.double().cpu(), rv.double().cpu()
        unb = var_ref * n / max(n - 1, 1)
        sd = var_ref.sqrt()
        rm_ref = (1 - momentum) * rm0.double() + momentum * mean_ref
        rv_ref = (1 - momentum) * rv0.double() + momentum * unb
        assert ((rm - rm_ref).abs() <= momentum * 5e-5 * sd + 4 * U * (rm0.abs() + mean_ref.abs())).all(), what
        assert ((rv - rv_ref).abs() <= momentum * 2e-4 * unb + 4 * U * (rv0.abs() + unb)).all(), what


def run_bn_stats(shape, place=place_aligned, affine=True, running=True):
    i = bn_inputs(shape)
    B, C, L = shape
    eps = 1e-5 if B * L == 1 else 0.0
    gamma, beta = (i['gamma'], i['beta']) if affine else (None, None)
    rm, rv = (dev(i['rm']).clone(), dev(i['rv']).clone()) if running else (None, None)
    xg = place('x', i['x'])
    poison(C)
    got = ops.bn_stats(xg, dev(gamma), dev(beta), eps, 0.1, rm, rv)
    check_stats('bn_stats {}'.format(shape), shape, got, i['x'], gamma, beta, eps, i['rm'], i['rv'],
                rm, rv)
    # emu_ops restates the same contract
    want = E.bn_stats(i['x'], gamma, beta, eps, 0.1, None, None)
    check_stats('emu bn_stats {}'.format(shape), shape, want, i['x'], gamma, beta, eps)
    return got


def chan_combine64(ws):
    """Chan et al. combination of partials [ns, C, 3] in float64 -> (n, mean, M2)."""
    w = ws.double().cpu()
    n = torch.zeros(w.shape[1], dtype=torch.float64)
    mean, m2 = torch.zeros_like(n), torch.zeros_like(n)
    for s in range(w.shape[0]):
        nb, mb, qb = w[s, :, 0], w[s, :, 1], w[s, :, 2]
        tot = (n + nb).clamp_min(1e-300)
        d = mb - mean
        mean = mean + d * nb / tot
        m2 = m2 + qb + d * d * n * nb / tot
        n = n + nb
    return n, mean, m2


def run_bn_partial_final(shape, place=place_aligned):
    i = bn_inputs(shape)
    B, C, L = shape
    eps = 1e-5 if B * L == 1 else 0.0
    ns = nsplit(B, C, L)
    per = -(-B // ns)
    xg = place('x', i['x'])
    poison(ns * C * 3)
    ws = ops.bn_partial(xg)
    no_nan(ws)
    assert tuple(ws.shape) == (ns, C, 3)
    rows = torch.tensor([max(0, min(B, (s + 1) * per) - s * per) for s in range(ns)])
    assert torch.equal(ws[:, :, 0].cpu(), (rows * L).float().view(ns, 1).expand(ns, C))
    rm, rv = dev(i['rm']).clone(), dev(i['rv']).clone()
    poison(C)
    got = ops.bn_final(ws, dev(i['gamma']), dev(i['beta']), eps, 0.1, rm, rv)
    check_stats('bn_partial+final {}'.format(shape), shape, got, i['x'], i['gamma'], i['beta'], eps,
                i['rm'], i['rv'], rm, rv)
    # bn_final alone: the same partials combined by emu_ops in float64 (a combination of ns
    # numbers in double: fp32 output rounding only)
    want = E.bn_final(ws.cpu(), i['gamma'], i['beta'], eps, 0.1, None, None)
    for k, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
        check_elem('bn_final {} {}'.format(name, shape), got[k], want[k], 1e-6)
    return ws


@pytest.mark.parametrize('shape', SHAPES)
def test_bn_stats_grid(shape):
    run_bn_stats(shape)
    run_bn_partial_final(shape)


def test_bn_stats_optional_arguments():
    for shape in ((5, 3, 1001), (300, 64, 16)):
        run_bn_stats(shape, affine=False)
        run_bn_stats(shape, running=False)
        run_bn_stats(shape, affine=False, running=False)


@pytest.mark.parametrize('shape', UNALIGNED_SHAPES)
def test_bn_stats_unaligned_views(shape):
    for off in (1, 2, 3):
        run_bn_stats(shape, place=place_unaligned('x', off))
        run_bn_partial_final(shape, place=place_unaligned('x', off))


def test_bn_final_combines_two_ranks():
    """bn_final over nsplit_total = 2 x nsplit partials (synchronised BatchNorm): the statistics
    of the concatenated batch."""
    shape = (300, 64, 16)
    x0 = bn_inputs(shape)['x']
    x1 = x0.flip(0) * 1.5 + 2.0
    ws = torch.cat((ops.bn_partial(dev(x0)), ops.bn_partial(dev(x1))), 0).contiguous()
    got = ops.bn_final(ws, None, None, 0.0, 0.1, None, None)
    check_stats('bn_final two ranks', (600, 64, 16), got, torch.cat((x0, x1), 0), None, None, 0.0)


def one_hot_positions(shape):
    """(b, c, t) of the probes: element 0; the last element of a row; the first element behind the
    float4 body of a row (4 * (L // 4), when L % 4 != 0); the last row of the first batch split;
    the last batch entry; the last element of the tensor."""
    B, C, L = shape
    per = -(-B // nsplit(B, C, L))
    pos = [(0, 0, 0), (0, C // 2, L - 1), (per - 1, C // 2, 0), (B - 1, C // 2, 0),
           (B - 1, C - 1, L - 1)]
    if L % 4:
        pos.append((B // 2, C // 2, 4 * (L // 4)))
    return sorted(set(pos))


@pytest.mark.parametrize('shape', ONE_HOT_SHAPES)
def test_bn_partial_one_hot(shape):
    """x zero but for one element x0: mean = x0 / n and M2 = x0^2 (1 - 1/n) in its channel, exactly
    zero in every other."""
    B, C, L = shape
    n = B * L
    m, ns = chan_m(B, C, L)
    x0 = 3.0
    for (b, c, t) in one_hot_positions(shape):
        x = torch.zeros(B, C, L, device=DEV)
        x[b, c, t] = x0
        poison(ns * C * 3)
        ws = ops.bn_partial(x)
        no_nan(ws)
        cnt, mean, m2 = chan_combine64(ws)
        assert (cnt == n).all()
        hot = torch.zeros(C, dtype=torch.float64)
        hot[c] = 1.0
        # the mean is a sum of one term x0 / n; M2 = s2 - s1^2 / n per thread and Chan merges of
        # (count, mean, M2): every merge adds a few roundings of magnitude x0^2, as a sum would
        check_sum('bn_partial one-hot mean {} {}'.format(shape, (b, c, t)), mean, hot * x0 / n,
                  sum_tol(hot * x0 / n, m, ns))
        check_sum('bn_partial one-hot M2 {} {}'.format(shape, (b, c, t)), m2,
                  hot * x0 * x0 * (1 - 1.0 / n), sum_tol(hot * x0 * x0, m, ns))


# ---------------------------------------------------------------------------------------------
# activation backward: plain PReLU, PReLU + skip, BatchNorm + PReLU
# ---------------------------------------------------------------------------------------------
def bn_v(a, mean, rstd, gamma, beta):
    """The fp64 gate argument of the BN form and its parts."""
    C = a.shape[1]
    mu, rs = mean.double().view(1, C, 1), rstd.double().view(1, C, 1)
    ga = gamma.double().view(1, C, 1) if gamma is not None else torch.ones(1, C, 1, dtype=torch.float64)
    be = beta.double().view(1, C, 1) if beta is not None else torch.zeros(1, C, 1, dtype=torch.float64)
    xh = (a.double() - mu) * rs
    return ga * xh + be, xh, ga, be, mu, rs


@functools.lru_cache(maxsize=6)
def act_inputs(form, shape, affine=True):
    """Gate-safe inputs of one act_bwd form ('prelu', 'skip', 'bn') on CPU."""
    B, C, L = shape
    a = rnd(B, C, L, seed=31) * 2 + 0.3
    i = dict(dh=rnd(B, C, L, seed=32), dskip=None, alpha=None, bn=None,
             slope=rnd(C, seed=33).abs() * 0.3)
    i['slope'][0] = 0.0                    # PReLU initialised at 0 (modules.py:81)
    if form == 'skip':
        i['dskip'], i['alpha'] = rnd(B, C, L, seed=34), rnd(C, seed=35)
    if form == 'bn':
        mean = 0.3 + 0.2 * rnd(C, seed=36)
        rstd = 0.5 * (1 + 0.4 * uni(C, seed=37))
        gamma = (0.5 + uni(C, seed=38)) * torch.where(torch.arange(C) % 3 == 1, -1.0, 1.0)
        beta = 0.5 * rnd(C, seed=39)
        if not affine:
            gamma = beta = None
        v, xh, ga, be, mu, rs = bn_v(a, mean, rstd, gamma, beta)
        a, frac = nudge(a, v, ga * rs, 2 * GATE)
        i['bn'] = (mean, rstd, gamma, beta)
        v = bn_v(a, *i['bn'])[0]
    else:
        a, frac = nudge(a, a.double(), 1.0, GATE)
        v = a.double()
    i['a'], i['v'], i['nudged'] = a, v, frac
    return i


def act_sums(form, i, dh, dskip, slope, count=None):
    """fp64 S = sum |term| per channel of every reduced output of act_bwd (module docstring);
    also the fp64 sums themselves where a bar needs them."""
    a, v = i['a'].double(), i['v']
    C = a.shape[1]
    dhd = dh.double() if dh is not None else torch.zeros_like(a)
    sl = slope.double().view(1, C, 1) if slope is not None else torch.ones(1, C, 1, dtype=torch.float64)
    gate = torch.where(v > 0, torch.ones_like(v), sl.expand_as(v))
    neg = (v <= 0).double()
    S = {}
    if form != 'bn':
        S['dslope'] = (dhd * a * neg).abs().sum((0, 2))
        g = (dhd * gate).abs()
        if dskip is not None:
            S['dalpha'] = (dskip.double() * a).abs().sum((0, 2))
            # g = fma(alpha, dskip, dh * gate) cancels: magnitudes before the cancellation
            g = g + (i['alpha'].double().view(1, C, 1) * dskip.double()).abs()
        S['dbias'] = g.sum((0, 2))
        return S
    _, xh, ga, be, mu, rs = bn_v(i['a'], *i['bn'])
    n = a.shape[0] * a.shape[2] if count is None else count
    sc = ga * rs
    sh = be - mu * sc
    g = dhd * gate
    # v = fmaf(a, scale, shift) with fp32 scale / shift cancels: |dh| (|a scale| + |shift|)
    S['dslope'] = (dhd.abs() * ((a * sc).abs() + sh.abs()) * neg).sum((0, 2))
    S['dbeta'] = g.abs().sum((0, 2))
    S['dgamma'] = (g.abs() * (a.abs() + mu.abs()) * rs).sum((0, 2))
    db, dg = g.sum((0, 2)).view(1, C, 1), (g * xh).sum((0, 2)).view(1, C, 1)
    S['dbias'] = (sc.abs() * (g.abs() + db.abs() / n + (a.abs() + mu.abs()) * rs * dg.abs() / n)).sum((0, 2))
    S['_sc'], S['_mean_abs_xh'] = sc.abs().view(-1), xh.abs().mean((0, 2))
    return S


ACT_GRADS = {'prelu': ('dslope', 'dbias'), 'skip': ('dslope', 'dalpha', 'dbias'),
             'bn': ('dslope', 'dgamma', 'dbeta', 'dbias')}


def run_act_bwd(form, shape, place=place_aligned, affine=True, dh_none=False, slope_none=False,
                outs=None, calls=1, prefill=False):
    """ops.act_bwd against emu_ops.act_bwd.  `outs`: the d* tensors passed (default: all the
    form has); `calls` > 1 and `prefill` test the accumulate-into rule.  Returns da."""
    B, C, L = shape
    i = act_inputs(form, shape, affine)
    assert i['v'].abs().min().item() >= GATE          # gate-safe on the reference side
    dh = None if dh_none else i['dh']
    slope = None if slope_none else i['slope']
    outs = ACT_GRADS[form] if outs is None else outs
    if slope is None:
        outs = tuple(o for o in outs if o != 'dslope')
    start = (0.5 + (torch.arange(C) % 3).float()) if prefill else torch.zeros(C)
    # reference
    ref = {o: torch.zeros(C, dtype=torch.float64) for o in ACT_GRADS[form]}
    da_ref = E.act_bwd(i['a'], dh, dskip=i['dskip'], slope=slope, alpha=i['alpha'], bn=i['bn'],
                       **{o: ref[o] for o in ref if not (o == 'dslope' and slope is None)})
    # GPU
    ag, dhg, dsg = place('a', i['a']), place('dh', dh), place('dskip', i['dskip'])
    bng = tuple(dev(t) for t in i['bn']) if i['bn'] is not None else None
    got = {o: dev(start).clone() for o in outs}
    for _ in range(calls):
        poison(B * C * L)
        da = ops.act_bwd(ag, dhg, dskip=dsg, slope=dev(slope), alpha=dev(i['alpha']), bn=bng, **got)
    no_nan(da)
    what = 'act_bwd[{}] {} affine={} dh_none={} slope_none={}'.format(form, shape, affine, dh_none,
                                                                    slope_none)
    check_elem(what + ' da', da, da_ref, 2e-5 if form == 'bn' else 1e-5)
    S = act_sums(form, i, dh, i['dskip'], slope)
    m, ns = chan_m(B, C, L)
    for o in outs:
        tol = sum_tol(S[o], m, ns)
        if form == 'bn' and o == 'dbias':
            # da depends on the fp32 totals (dbeta, dgamma) / n: their own error enters every
            # element of the channel: |scale| (tol_dbeta + mean|xhat| tol_dgamma)
            tol = tol + S['_sc'] * (sum_tol(S['dbeta'], m, ns)
                                    + S['_mean_abs_xh'] * sum_tol(S['dgamma'], m, ns))
        # every `+=` into a non-zero accumulator rounds once more, at the accumulator's size
        inexact = calls - (0 if prefill else 1)
        tol = calls * tol + inexact * 2 * U * (start.double() + calls * S[o])
        check_sum(what + ' ' + o, got[o], start.double() + calls * ref[o], tol)
    return da


ACT_FORMS = ('prelu', 'skip', 'bn')


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('form', ACT_FORMS)
def test_act_bwd_grid(form, shape):
    run_act_bwd(form, shape)
    if shape == BIG:
        # about 5e-4 of the elements of a ~ 2 N(0, 1) + 0.3 lie within 1e-3 of the gate
        assert act_inputs(form, shape)['nudged'] < 2e-3


@pytest.mark.parametrize('form', ACT_FORMS)
def test_act_bwd_optional_arguments(form):
    for shape in ((5, 3, 1001), (300, 64, 16)):
        run_act_bwd(form, shape, slope_none=True)
        names = ACT_GRADS[form]
        for k in range(len(names)):                     # each d* output None in turn
            run_act_bwd(form, shape, outs=names[:k] + names[k + 1:])
        run_act_bwd(form, shape, outs=())
        if form == 'skip':
            run_act_bwd(form, shape, dh_none=True)
            run_act_bwd(form, shape, dh_none=True, slope_none=True)
        if form == 'bn':
            run_act_bwd(form, shape, affine=False)
            run_act_bwd(form, shape, affine=False, slope_none=True)


def test_act_bwd_forbidden_combinations_raise():
    i = act_inputs('skip', (5, 5, 8))
    b = act_inputs('bn', (5, 5, 8))
    a, dh, ds = dev(i['a']), dev(i['dh']), dev(i['dskip'])
    bn = tuple(dev(t) for t in b['bn'])
    with pytest.raises(RuntimeError, match='dskip needs alpha'):
        ops.act_bwd(a, dh, dskip=ds, slope=dev(i['slope']))
    with pytest.raises(RuntimeError, match='no skip tap'):
        ops.act_bwd(a, dh, dskip=ds, slope=dev(i['slope']), alpha=dev(i['alpha']), bn=bn)
    with pytest.raises(RuntimeError, match='no incoming gradient'):
        ops.act_bwd(a, None, slope=dev(i['slope']))
    with pytest.raises(RuntimeError, match='no incoming gradient'):
        ops.tanh_bwd(a, None)
    with pytest.raises(RuntimeError, match='NULL pointer'):
        ops.act_bwd_bn_reduce(a, None, dev(i['slope']), bn)
    torch.cuda.synchronize()


@pytest.mark.parametrize('shape', ((5, 3, 1001), (300, 64, 16), (300, 8, 4096)))
@pytest.mark.parametrize('form', ACT_FORMS)
def test_act_bwd_accumulates(form, shape):
    run_act_bwd(form, shape, calls=2, prefill=True)


@pytest.mark.parametrize('shape', UNALIGNED_SHAPES)
@pytest.mark.parametrize('form', ACT_FORMS)
def test_act_bwd_unaligned_views(form, shape):
    """The scalar path taken for a base pointer off a 16-byte boundary: sums and the BN da at
    the bars of the aligned call, the other da bit-equal to it."""
    base = run_act_bwd(form, shape)
    for off in (1, 2, 3):
        for which in ('a', 'dh', 'dskip', 'all'):
            if which == 'dskip' and form != 'skip':
                continue
            da = run_act_bwd(form, shape, place=place_unaligned(which, off))
            if form != 'bn':
                assert torch.equal(da, base), (form, which, off)


def one_element(i, c, v_want):
    """The inputs `i` cut down to one element of channel c whose gate argument is v_want."""
    j = dict(i)
    j['slope'] = i['slope'][c:c + 1]
    j['alpha'] = None if i['alpha'] is None else i['alpha'][c:c + 1]
    if i['bn'] is None:
        j['bn'] = None
        j['a'] = torch.tensor(v_want, dtype=torch.float32).view(1, 1, 1)
        j['v'] = j['a'].double()
    else:
        j['bn'] = tuple(t[c:c + 1] for t in i['bn'])
        mean, rstd, gamma, beta = (t.double() for t in j['bn'])
        j['a'] = (mean + (v_want - beta) / (gamma * rstd)).float().view(1, 1, 1)
        j['v'] = bn_v(j['a'], *j['bn'])[0]
    assert j['v'].abs().min().item() >= GATE
    return j


@pytest.mark.parametrize('shape', ONE_HOT_SHAPES)
@pytest.mark.parametrize('form', ACT_FORMS)
def test_act_bwd_one_hot(form, shape):
    """Incoming gradient zero but for one element, on either side of the gate: every per-channel
    sum is that one term, and exactly zero in the other channels."""
    B, C, L = shape
    i = act_inputs(form, shape)
    m, ns = chan_m(B, C, L)
    ag = dev(i['a']).clone()
    bng = tuple(dev(t) for t in i['bn']) if i['bn'] is not None else None
    g0, s0 = 1.75, -0.625
    for k, (b, c, t) in enumerate(one_hot_positions(shape)):
        for v_want in (0.8, -0.6):
            j = one_element(i, c, v_want)
            keep = ag[b, c, t].item()
            ag[b, c, t] = j['a'].item()
            dh = torch.zeros(B, C, L, device=DEV)
            dh[b, c, t] = g0
            dsk = None
            if form == 'skip':
                dsk = torch.zeros(B, C, L, device=DEV)
                dsk[b, c, t] = s0
            got = {o: torch.zeros(C, device=DEV) for o in ACT_GRADS[form]}
            poison(B * C * L)
            da = ops.act_bwd(ag, dh, dskip=dsk, slope=dev(i['slope']), alpha=dev(i['alpha']),
                             bn=bng, **got)
            no_nan(da)
            ag[b, c, t] = keep
            if form != 'bn':
                assert int((da != 0).sum()) <= 1
            # the reference on that one element
            dh1 = torch.full((1, 1, 1), g0)
            ds1 = torch.full((1, 1, 1), s0) if form == 'skip' else None
            ref = {o: torch.zeros(1, dtype=torch.float64) for o in ACT_GRADS[form]}
            E.act_bwd(j['a'], dh1, dskip=ds1, slope=j['slope'], alpha=j['alpha'], bn=j['bn'], **ref)
            S = act_sums(form, j, dh1, ds1, j['slope'])
            what = 'act_bwd[{}] one-hot {} at {} v={}'.format(form, shape, (b, c, t), v_want)
            for o in ACT_GRADS[form]:
                if form == 'bn' and o == 'dbias':
                    continue       # a sum over every element of the channel, not one term
                want, tol = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
                want[c], tol[c] = ref[o][0], sum_tol(S[o][0], m, ns)
                check_sum(what + ' ' + o, got[o], want, tol)


# ---- the BatchNorm branch in two calls --------------------------------------------------------
def run_bn_two_calls(shape, place=place_aligned, affine=True, slope_none=False, calls=1,
                     prefill=False, outs=('dslope', 'dgamma', 'dbeta')):
    B, C, L = shape
    i = act_inputs('bn', shape, affine)
    assert i['v'].abs().min().item() >= GATE
    slope = None if slope_none else i['slope']
    if slope is None:
        outs = tuple(o for o in outs if o != 'dslope')
    start = (0.5 + (torch.arange(C) % 3).float()) if prefill else torch.zeros(C)
    ref = {o: torch.zeros(C, dtype=torch.float64) for o in ('dslope', 'dgamma', 'dbeta')}
    tot_ref, _ = E.act_bwd_bn_reduce(i['a'], i['dh'], slope, i['bn'], **ref)
    ag, dhg = place('a', i['a']), place('dh', i['dh'])
    bng = tuple(dev(t) for t in i['bn'])
    got = {o: dev(start).clone() for o in outs}
    for _ in range(calls):
        poison(2 * C)
        totals, ws = ops.act_bwd_bn_reduce(ag, dhg, dev(slope), bng, **got)
    no_nan(totals)
    S = act_sums('bn', i, i['dh'], None, slope)
    m, ns = chan_m(B, C, L)
    what = 'act_bwd_bn_reduce {} affine={} slope_none={}'.format(shape, affine, slope_none)
    for o in outs:
        inexact = calls - (0 if prefill else 1)
        tol = calls * sum_tol(S[o], m, ns) + inexact * 2 * U * (start.double() + calls * S[o])
        check_sum(what + ' ' + o, got[o], start.double() + calls * ref[o], tol)
    check_sum(what + ' totals[:, 0]', totals[:, 0], ref['dbeta'], sum_tol(S['dbeta'], m, ns))
    check_sum(what + ' totals[:, 1]', totals[:, 1], ref['dgamma'], sum_tol(S['dgamma'], m, ns))
    # apply: the GPU's own totals as the (all-reduced) input of both sides; a global count of two
    # ranks' worth on a second call
    for count, reuse_ws in ((B * L, True), (2 * B * L, False)):
        dbi = dev(start).clone()
        for _ in range(calls):
            poison(B * C * L)
            da = ops.act_bwd_bn_apply(ag, dhg, dev(slope), bng, totals, count, dbias=dbi,
                                      ws=ws if reuse_ws else None)
        no_nan(da)
        dbi_ref = torch.zeros(C, dtype=torch.float64)
        da_ref = E.act_bwd_bn_apply(i['a'], i['dh'], slope, i['bn'], totals.cpu(), count,
                                    dbias=dbi_ref)
        check_elem(what + ' apply da count={}'.format(count), da, da_ref, 2e-5)
        inexact = calls - (0 if prefill else 1)
        Sb = act_sums('bn', i, i['dh'], None, slope, count)['dbias']
        tol = calls * sum_tol(Sb, m, ns) + inexact * 2 * U * (start.double() + calls * Sb)
        check_sum(what + ' apply dbias count={}'.format(count), dbi,
                  start.double() + calls * dbi_ref, tol)
    ops.act_bwd_bn_apply(ag, dhg, dev(slope), bng, totals, B * L)          # dbias None


@pytest.mark.parametrize('shape', SHAPES)
def test_act_bwd_bn_reduce_apply_grid(shape):
    run_bn_two_calls(shape)


def test_act_bwd_bn_reduce_apply_options():
    for shape in ((5, 3, 1001), (300, 64, 16)):
        run_bn_two_calls(shape, affine=False)
        run_bn_two_calls(shape, slope_none=True)
        run_bn_two_calls(shape, outs=())
        run_bn_two_calls(shape, outs=('dgamma',))
        run_bn_two_calls(shape, calls=2, prefill=True)
    for shape in UNALIGNED_SHAPES:
        for off in (1, 2, 3):
            for which in ('a', 'dh', 'all'):
                run_bn_two_calls(shape, place=place_unaligned(which, off))


# ---------------------------------------------------------------------------------------------
# tanh backward
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def tanh_inputs(shape):
    B, C, L = shape
    y = torch.tanh(rnd(B, C, L, seed=41))
    clean = rnd(B, C, L, seed=42).clamp(-1, 1)
    clean.view(-1)[::7] = y.view(-1)[::7]          # sign(0) = 0
    return dict(y=y, dy=rnd(B, C, L, seed=43), clean=clean)


def tanh_S(y, dy, clean, l1):
    """|term| of tanh_bwd's dbias before the cancellations of its fp32 expression
    (dy + l1 sign(y - clean)) (1 - y y): (|dy| + l1 |sign|) (1 + y y)."""
    yd = y.double()
    g = dy.double().abs() if dy is not None else torch.zeros_like(yd)
    if clean is not None:
        g = g + l1 * torch.sign(yd - clean.double()).abs()
    return g * (1 + yd * yd)


def run_tanh_bwd(shape, place=place_aligned, dy_none=False, clean_none=False, dbias=True, calls=1,
                 prefill=False):
    B, C, L = shape
    i = tanh_inputs(shape)
    dy = None if dy_none else i['dy']
    clean = None if clean_none else i['clean']
    l1 = 0.25
    start = (0.5 + (torch.arange(C) % 3).float()) if prefill else torch.zeros(C)
    ref = torch.zeros(C, dtype=torch.float64)
    da_ref = E.tanh_bwd(i['y'], dy, clean=clean, l1_scale=l1, dbias=ref)
    yg, dyg, cg = place('y', i['y']), place('dy', dy), place('clean', clean)
    db = dev(start).clone() if dbias else None
    for _ in range(calls):
        poison(B * C * L)
        da = ops.tanh_bwd(yg, dyg, clean=cg, l1_scale=l1, dbias=db)
    no_nan(da)
    what = 'tanh_bwd {} dy_none={} clean_none={}'.format(shape, dy_none, clean_none)
    check_elem(what + ' da', da, da_ref)
    if dbias:
        S = tanh_S(i['y'], dy, clean, l1).sum((0, 2))
        m, ns = chan_m(B, C, L)
        inexact = calls - (0 if prefill else 1)
        tol = calls * sum_tol(S, m, ns) + inexact * 2 * U * (start.double() + calls * S)
        check_sum(what + ' dbias', db, start.double() + calls * ref, tol)
    return da


@pytest.mark.parametrize('shape', SHAPES)
def test_tanh_bwd_grid(shape):
    run_tanh_bwd(shape)


def test_tanh_bwd_optional_arguments_and_accumulation():
    for shape in ((5, 3, 1001), (300, 64, 16), (300, 1, 1001)):
        run_tanh_bwd(shape, dy_none=True)
        run_tanh_bwd(shape, clean_none=True)
        run_tanh_bwd(shape, dbias=False)
        run_tanh_bwd(shape, calls=2, prefill=True)
    run_tanh_bwd(BIG, calls=2, prefill=True)


@pytest.mark.parametrize('shape', UNALIGNED_SHAPES)
def test_tanh_bwd_unaligned_views(shape):
    base = run_tanh_bwd(shape)
    for off in (1, 2, 3):
        for which in ('y', 'dy', 'clean', 'all'):
            da = run_tanh_bwd(shape, place=place_unaligned(which, off))
            assert torch.equal(da, base), (which, off)


@pytest.mark.parametrize('shape', ONE_HOT_SHAPES)
def test_tanh_bwd_one_hot(shape):
    B, C, L = shape
    y = tanh_inputs(shape)['y']
    yg = dev(y)
    m, ns = chan_m(B, C, L)
    for (b, c, t) in one_hot_positions(shape):
        dy = torch.zeros(B, C, L, device=DEV)
        dy[b, c, t] = 1.75
        db = torch.zeros(C, device=DEV)
        poison(B * C * L)
        da = ops.tanh_bwd(yg, dy, dbias=db)
        no_nan(da)
        want = torch.zeros(C, dtype=torch.float64)
        want[c] = 1.75 * (1 - y[b, c, t].double() ** 2)
        S = torch.zeros(C, dtype=torch.float64)
        S[c] = 1.75 * (1 + y[b, c, t].double() ** 2)
        check_sum('tanh_bwd one-hot {} at {}'.format(shape, (b, c, t)), db, want,
                  sum_tol(S, m, ns))
        assert int((da != 0).sum()) <= 1


# ---------------------------------------------------------------------------------------------
# dense head: bias + PReLU over [rows, cols]
# ---------------------------------------------------------------------------------------------
ROWS = (1, 3, 4, 5, 300)
COLS = (1, 63, 64, 65, 256)


@functools.lru_cache(maxsize=None)
def rows_inputs(rows, cols, has_bias):
    x = rnd(rows, cols, seed=51) + 0.2
    bias = rnd(cols, seed=52) if has_bias else None
    v = x.double() + (bias.double() if has_bias else 0.0)
    x, _ = nudge(x, v, 1.0, 2 * GATE)
    v = x.double() + (bias.double() if has_bias else 0.0)
    slope = rnd(cols, seed=53).abs() * 0.3
    return dict(x=x, bias=bias, slope=slope, dy=rnd(rows, cols, seed=54), v=v)


def run_rows(rows, cols, has_bias=True, has_slope=True, outs=('dslope', 'dbias'), calls=1,
             prefill=False):
    i = rows_inputs(rows, cols, has_bias)
    assert i['v'].abs().min().item() >= GATE
    slope = i['slope'] if has_slope else None
    what = 'bias_prelu_rows {}x{} bias={} slope={}'.format(rows, cols, has_bias, has_slope)
    xg = dev(i['x'])
    poison(rows * cols)
    y = ops.bias_prelu_rows(xg, dev(i['bias']), dev(slope))
    no_nan(y)
    check_elem(what + ' y', y, E.bias_prelu_rows(i['x'], i['bias'], slope))
    start = (0.5 + (torch.arange(cols) % 3).float()) if prefill else torch.zeros(cols)
    ref = {o: torch.zeros(cols, dtype=torch.float64) for o in ('dslope', 'dbias')}
    dx_ref = E.bias_prelu_rows_bwd(i['x'], i['bias'], slope, i['dy'], ref['dslope'], ref['dbias'])
    got = {o: (dev(start).clone() if o in outs else None) for o in ('dslope', 'dbias')}
    for _ in range(calls):
        poison(rows * cols)
        dx = ops.bias_prelu_rows_bwd(xg, dev(i['bias']), dev(slope), dev(i['dy']), got['dslope'],
                                     got['dbias'])
    no_nan(dx)
    check_elem(what + ' dx', dx, dx_ref)
    # 4 row groups walk the rows (m = ceil(rows / 4)) and are added in LDS; no second pass
    m = -(-rows // 4)
    S = {'dslope': (i['dy'].double() * i['v'] * (i['v'] <= 0)).abs().sum(0) if has_slope
         else torch.zeros(cols, dtype=torch.float64),
         'dbias': dx_ref.double().abs().sum(0)}
    for o in outs:
        inexact = calls - (0 if prefill else 1)
        tol = calls * sum_tol(S[o], m, 0) + inexact * 2 * U * (start.double() + calls * S[o])
        check_sum(what + ' ' + o, got[o], start.double() + calls * ref[o], tol)


@pytest.mark.parametrize('cols', COLS)
@pytest.mark.parametrize('rows', ROWS)
def test_bias_prelu_rows_grid(rows, cols):
    for has_bias in (True, False):
        for has_slope in (True, False):
            run_rows(rows, cols, has_bias, has_slope)


def test_bias_prelu_rows_outputs_optional_and_accumulate():
    for rows, cols in ((5, 65), (300, 256)):
        run_rows(rows, cols, outs=('dslope',))
        run_rows(rows, cols, outs=('dbias',))
        run_rows(rows, cols, outs=())
        run_rows(rows, cols, calls=2, prefill=True)


def test_bias_prelu_rows_large():
    """The forward's grid-stride loop behind its 2048 x 256 cap: 2.2 M elements, 5 trips."""
    run_rows(5000, 431)


@pytest.mark.parametrize('rows,cols', [(300, 256), (5, 65), (3, 1)])
def test_bias_prelu_rows_bwd_one_hot(rows, cols):
    i = rows_inputs(rows, cols, True)
    xg, bg, sg = dev(i['x']), dev(i['bias']), dev(i['slope'])
    for (r, c) in sorted({(0, 0), (rows - 1, cols // 2), (rows // 2, cols - 1),
                          (rows - 1, cols - 1), (min(3, rows - 1), 0)}):
        dy = torch.zeros(rows, cols, device=DEV)
        dy[r, c] = 1.75
        ds, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
        poison(rows * cols)
        ops.bias_prelu_rows_bwd(xg, bg, sg, dy, ds, db)
        v = i['v'][r, c].item()
        want_s, want_b = torch.zeros(cols, dtype=torch.float64), torch.zeros(cols, dtype=torch.float64)
        want_s[c] = 1.75 * min(v, 0.0)
        want_b[c] = 1.75 * (1.0 if v > 0 else i['slope'][c].item())
        m = -(-rows // 4)
        check_sum('rows one-hot dslope {}x{} at {}'.format(rows, cols, (r, c)), ds, want_s,
                  sum_tol(want_s.abs(), m, 0))
        check_sum('rows one-hot dbias {}x{} at {}'.format(rows, cols, (r, c)), db, want_b,
                  sum_tol(want_b.abs(), m, 0))


# ---------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------
FLAT_N = (1, 3, 255, 256, 257, 1048576 + 3, 2 * 2048 * 256 * 4 + 5)


def flat_m(n, cap):
    """Terms one thread adds in a flat grid-stride reduction capped at `cap` workgroups, and the
    serial terms of the one-workgroup final pass over the per-workgroup partials."""
    blocks = min(cap, -(-n // 256))
    return -(-n // (blocks * 256)), -(-blocks // 256)


@pytest.mark.parametrize('n', FLAT_N)
def test_l1_mse_mean_and_bwd(n):
    x, y = rnd(n, seed=61), rnd(n, seed=62)
    y[::5] = x[::5]                         # sign(0) = 0
    xg, yg = dev(x), dev(y)
    m, fin = flat_m(n, 1024)
    for name in ('l1', 'mse'):
        mean, bwd = getattr(ops, name + '_mean'), getattr(ops, name + '_bwd')
        emean, ebwd = getattr(E, name + '_mean'), getattr(E, name + '_bwd')
        poison(1)
        got = mean(xg, yg)
        d = x.double() - y.double()
        S = (d.abs() if name == 'l1' else d * d).sum().item() / n
        check_sum('{}_mean n={}'.format(name, n), got,
                  (d.abs() if name == 'l1' else d * d).sum() / n, sum_tol(S, m, fin))
        check_elem('{}_mean vs emu n={}'.format(name, n), got.view(1), emean(x, y).view(1), 1e-5)
        for gout, gscale in ((None, 1.0), (None, 100.0), (torch.tensor([0.75]), 1.0),
                             (torch.tensor([-3.0]), 0.5)):
            poison(n)
            g = bwd(xg, yg, gout=dev(gout), gscale=gscale)
            no_nan(g)
            check_elem('{}_bwd n={} gout={} gscale={}'.format(name, n, gout, gscale), g,
                       ebwd(x, y, gout=gout, gscale=gscale))


@pytest.mark.parametrize('name', ('l1', 'mse'))
def test_l1_mse_mean_one_hot(name):
    mean = getattr(ops, name + '_mean')
    for n in (257, 1048576 + 3, 2 * 2048 * 256 * 4 + 5):
        m, fin = flat_m(n, 1024)
        base = rnd(n, seed=63)
        xg = dev(base)
        for pos in sorted({0, 255, 256, n // 2, min(n - 1, 1024 * 256), n - 1}):
            yg = xg.clone()
            yg[pos] += 1.5
            d = float(yg[pos].item()) - float(xg[pos].item())
            want = (abs(d) if name == 'l1' else d * d) / n
            poison(1)
            got = mean(xg, yg)
            check_sum('{}_mean one-hot n={} at {}'.format(name, n, pos), got, want,
                      sum_tol(want, m, fin))


CONST_N = (1, 255, 256, 257, 300, 5000)


@pytest.mark.parametrize('n', CONST_N)
@pytest.mark.parametrize('kind', ('mse_const', 'bce_logits_const'))
def test_const_target_losses(kind, n):
    x = rnd(n, seed=71) * 3
    # -30 first: as the ONLY element (n = 1) of a max_rel comparison a logit must not be one where
    # sigmoid(x) - target cancels to below half an ulp of 1 in fp32 (x = 30 against target 1)
    edge = torch.tensor([-30.0, 30.0, 100.0, -100.0, 0.0])[:n]
    x[:edge.numel()] = edge
    xg = dev(x)
    fwd, bwd = getattr(ops, kind), getattr(ops, kind + '_bwd')
    efwd, ebwd = getattr(E, kind), getattr(E, kind + '_bwd')
    xd = x.double()
    for target in (0.0, 1.0):
        if kind == 'mse_const':
            terms = (xd - target) ** 2
        else:
            # max(x, 0) - x t is exact in fp32 for t in {0, 1} and every term is >= 0
            terms = xd.clamp_min(0) - xd * target + torch.log1p(torch.exp(-xd.abs()))
        assert torch.isfinite(terms).all()
        want = efwd(x, target)
        assert torch.isfinite(want)
        poison(1)
        got = fwd(xg, target)
        # one workgroup of 256 threads: m = ceil(n / 256), no second pass
        check_sum('{} n={} target={}'.format(kind, n, target), got, terms.mean(),
                  sum_tol(terms.abs().mean().item(), -(-n // 256), 0))
        check_elem('{} vs emu n={} target={}'.format(kind, n, target), got.view(1), want.view(1), 1e-5)
        for gout, gscale in ((None, 1.0), (None, 0.25), (torch.tensor([0.75]), 1.0),
                             (torch.tensor([-3.0]), 0.5)):
            poison(n)
            g = bwd(xg, target, gout=dev(gout), gscale=gscale)
            no_nan(g)
            assert torch.isfinite(g).all()
            check_elem('{}_bwd n={} target={} gout={} gscale={}'.format(kind, n, target, gout, gscale),
                       g, ebwd(x, target, gout=gout, gscale=gscale))


# ---------------------------------------------------------------------------------------------
# fill_, scale_, optimizers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', FLAT_N)
def test_fill_and_scale(n):
    x = rnd(n, seed=81)
    buf = torch.zeros(n + 8, device=DEV)
    t = buf[4:4 + n]
    t.copy_(x)
    assert ops.scale_(t, -0.3) is t
    assert torch.equal(t.cpu(), (x.double() * float(np.float32(-0.3))).float())   # one rounding
    ops.fill_(t, 1.25)
    assert torch.equal(t.cpu(), torch.full((n,), 1.25))
    # neither wrote outside its n elements
    assert float(buf[:4].abs().max()) == 0.0 and float(buf[4 + n:].abs().max()) == 0.0


def opt_inputs(n):
    # |p| < 1: an ulp of p is at most 6e-8 there, so that where two correctly rounded fp32
    # evaluation orders of the same update land on either side of a rounding boundary of p they
    # differ by less than the 2e-7 bar (at |p| >= 2 one ulp of p is 2.4e-7)
    p = (rnd(n, seed=91) * 0.3).clamp(-0.99, 0.99)
    gs = [rnd(n, seed=92 + k) for k in range(3)]
    return p, gs


@pytest.mark.parametrize('n', FLAT_N)
def test_rmsprop_step(n):
    p, gs = opt_inputs(n)
    sq = uni(n, seed=95)
    pg, sqg = dev(p).clone(), dev(sq).clone()
    pc, sqc = p.clone(), sq.clone()
    for g in gs:
        ops.rmsprop_step(pg, dev(g), sqg, 5e-5, 0.99, 1e-8)
        E.rmsprop_step(pc, g.clone(), sqc, 5e-5, 0.99, 1e-8)
    err = (pg.cpu() - pc).abs().max().item()
    print('rmsprop n={}: max |dp| = {:.3g} (bar 2e-7)'.format(n, err))
    assert err <= 2e-7
    check_elem('rmsprop square average n={}'.format(n), sqg, sqc.double())


def test_rmsprop_unaligned_arena_raises():
    n = 1024
    buf = torch.zeros(n + 4, device=DEV)
    g, sq = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for bad in ('p', 'g', 'sq'):
        args = dict(p=torch.zeros(n, device=DEV), g=g, sq=sq)
        args[bad] = buf[1:1 + n]
        with pytest.raises(RuntimeError, match='16-byte aligned'):
            ops.rmsprop_step(args['p'], args['g'], args['sq'], 5e-5, 0.99, 1e-8)
    torch.cuda.synchronize()


@pytest.mark.parametrize('betas', ((0.0, 0.9), (0.9, 0.999)))
@pytest.mark.parametrize('step0', (1, 1000))
@pytest.mark.parametrize('n', FLAT_N)
def test_adam_step(n, step0, betas):
    p, gs = opt_inputs(n)
    fresh = step0 == 1
    m = torch.zeros(n) if fresh else rnd(n, seed=96) * 0.1
    v = torch.zeros(n) if fresh else uni(n, seed=97) * 0.01 + 1e-4
    pg, mg, vg = dev(p).clone(), dev(m).clone(), dev(v).clone()
    pc, mc, vc = p.clone(), m.clone(), v.clone()
    for k, g in enumerate(gs):
        ops.adam_step(pg, dev(g), mg, vg, 5e-5, betas[0], betas[1], 1e-8, step0 + k)
        E.adam_step(pc, g.clone(), mc, vc, 5e-5, betas[0], betas[1], 1e-8, step0 + k)
    err = (pg.cpu() - pc).abs().max().item()
    print('adam n={} step0={} betas={}: max |dp| = {:.3g} (bar 2e-7)'.format(n, step0, betas, err))
    assert err <= 2e-7
    check_elem('adam m', mg, mc.double())
    check_elem('adam v', vg, vc.double())


@pytest.mark.parametrize('kind', ('rmsprop', 'adam'))
def test_optimizer_steps_match_torch_optim(kind):
    n = 1048576 + 3
    p, gs = opt_inputs(n)
    ref_p = torch.nn.Parameter(p.clone())
    pg = dev(p).clone()
    if kind == 'rmsprop':
        ref = torch.optim.RMSprop([ref_p], lr=5e-5)
        state = [torch.zeros(n, device=DEV)]
    else:
        ref = torch.optim.Adam([ref_p], lr=5e-5, betas=(0.0, 0.9))
        state = [torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    for k, g in enumerate(gs):
        ref_p.grad = g.clone()
        ref.step()
        if kind == 'rmsprop':
            ops.rmsprop_step(pg, dev(g), state[0], 5e-5, 0.99, 1e-8)
        else:
            ops.adam_step(pg, dev(g), state[0], state[1], 5e-5, 0.0, 0.9, 1e-8, k + 1)
    err = (pg.cpu() - ref_p.detach()).abs().max().item()
    print('{} vs torch.optim: max |dp| = {:.3g} (bar 2e-7)'.format(kind, err))
    assert err <= 2e-7


# ---------------------------------------------------------------------------------------------
# global pooling over time
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', (1, 63, 64, 65, 1000))
@pytest.mark.parametrize('B,C', ((3, 7), (1, 1), (2, 5)))
def test_pool_time(B, C, L):
    assert (B * C) % 4 != 0
    x = (rnd(B, C, L, seed=101) * 2).round() / 2          # a grid of values: many ties
    x[0, 0] = 0.75                                        # a constant row
    x[-1, -1, L // 2:] = x[-1, -1].max()                  # the maximum repeated to the end
    xm = x.clone()
    if B * C > 1:
        xm[0, -1] = float('-inf')                         # a row of -inf
    for mode, xin in (('max', xm), ('avg', x)):
        poison(B * C)
        y, idx = ops.pool_time_fwd(dev(xin), mode)
        no_nan(y)
        y_ref, idx_ref = E.pool_time_fwd(xin, mode)
        if mode == 'max':
            assert torch.equal(y.cpu(), y_ref)
            assert idx.dtype == torch.int32 and torch.equal(idx.cpu(), idx_ref)   # first index wins
            assert int(idx[0, 0]) == 0
        else:
            assert idx is None
            check_elem('pool_time_fwd avg', y, xin.double().mean(2))
            check_elem('emu pool_time_fwd avg', y_ref, xin.double().mean(2))
        dy = rnd(B, C, seed=102)
        poison(B * C * L)
        dx = ops.pool_time_bwd(dev(dy), idx, L, mode)
        no_nan(dx)
        dx_ref = E.pool_time_bwd(dy, idx_ref, L, mode)
        if mode == 'max':
            assert torch.equal(dx.cpu(), dx_ref)
        else:
            check_elem('pool_time_bwd avg', dx, dx_ref.double())


def test_pool_time_many_rows():
    """pool_time_bwd's grid-stride loop behind its cap: 2100 x 1001 = 2.1 M elements."""
    B, C, L = 3, 700, 1001
    x = (rnd(B, C, L, seed=103) * 2).round() / 2
    dy = rnd(B, C, seed=104)
    for mode in ('max', 'avg'):
        y, idx = ops.pool_time_fwd(dev(x), mode)
        y_ref, idx_ref = E.pool_time_fwd(x, mode)
        poison(B * C * L)
        dx = ops.pool_time_bwd(dev(dy), idx, L, mode)
        no_nan(dx)
        if mode == 'max':
            assert torch.equal(y.cpu(), y_ref) and torch.equal(idx.cpu(), idx_ref)
            assert torch.equal(dx.cpu(), E.pool_time_bwd(dy, idx_ref, L, mode))
        else:
            check_elem('pool_time_fwd avg rows', y, x.double().mean(2))
            check_elem('pool_time_bwd avg rows', dx, E.pool_time_bwd(dy, None, L, mode).double())


# ---------------------------------------------------------------------------------------------
# de-emphasis scan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coef', (0.95, 0.5))
@pytest.mark.parametrize('rows', (1, 300))
@pytest.mark.parametrize('T', (1, 7, 8, 9, 8191, 8192, 8193, 16384, 3 * 8192 + 5))
def test_de_emphasize(T, rows, coef):
    from scipy.signal import lfilter
    y = uni(rows, T, seed=111) * 2 - 1                    # |y| <= 1
    want = lfilter([1.0], [1.0, -coef], y.numpy().astype(np.float64), axis=-1)
    yg = dev(y)
    poison(rows * T)
    x = ops.de_emphasize(yg, coef)
    no_nan(x)
    err = np.abs(x.cpu().numpy().astype(np.float64) - want).max()
    print('de_emphasize T={} rows={} coef={}: max |err| = {:.3g} (bar 5e-6)'.format(T, rows, coef, err))
    assert x.shape == y.shape
    assert err <= 5e-6
    # rows are independent: a row of the batch call is bit-equal to its single-row call
    for r in sorted({0, rows // 2 - 13 if rows > 1 else 0, rows - 1}):
        single = ops.de_emphasize(yg[r:r + 1].contiguous(), coef)
        assert torch.equal(single[0], x[r]), r
