"""Parity of every HIP entry point with the CPU oracle / torch fp64 on seeded inputs.

Tolerance: the kernels are exact fp32 (MFMA f32 == fmaf chain); against an fp64
reference the error is fp32 accumulation roundoff.  Bar used here: max|err| <= 3e-5 *
max|ref| for the contractions (K' up to ~16k terms), 1e-5 for pointwise kernels.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import segan_oracle as O
from conftest import max_rel

pytestmark = pytest.mark.gpu

TOL = 3e-5
DEV = 'cuda'


def _ops():
    from segan_pytorch_amd import ops
    return ops


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def xform_ref(x, scale=None, shift=None, slope=None):
    x = x.double()
    if scale is not None:
        x = x * scale.double().view(1, -1, 1)
    if shift is not None:
        x = x + shift.double().view(1, -1, 1)
    if slope is not None:
        x = torch.where(x > 0, x, x * slope.double().view(1, -1, 1))
    return x


def conv_ref(x, w, b, S, roll=0):
    K = w.shape[2]
    P = (K // 2 - 1, K // 2) if S > 1 else (K // 2, K // 2)
    xr = O.roll(x, roll)
    return F.conv1d(F.pad(xr, P, mode='reflect'), w, b, stride=S)


CONV_CASES = [
    # B, N(Cin), M(Cout), L, S, K, roll
    (2, 3, 5, 64, 4, 31, 0),
    (3, 64, 128, 256, 4, 31, 2),
    (2, 2, 64, 1024, 4, 31, -3),
    (5, 1, 64, 256, 4, 31, 0),
    (9, 32, 200, 64, 4, 31, 5),
    (2, 16, 24, 128, 2, 31, -1),
    (3, 8, 8, 64, 1, 31, 0),
    (2, 6, 7, 128, 4, 5, 1),
    (2, 256, 130, 512, 4, 31, 0),
    (1, 12, 40, 4096, 4, 31, 4),
    # stride 2 with few channels: the small-row tiles (F 32 x 256; T 64 / 32 rows; W 64 / 32 rows)
    (3, 16, 32, 512, 2, 31, 2),
    (2, 32, 32, 1024, 2, 31, -3),
    (3, 32, 64, 256, 2, 31, 1),
    (5, 12, 20, 64, 2, 31, 0),
    (2, 16, 32, 16, 2, 31, 0),
    (2, 20, 48, 2048, 2, 31, 5),
]


@pytest.mark.parametrize('B,N,M,L,S,K,roll', CONV_CASES)
def test_conv1d_fwd_dgrad_wgrad(B, N, M, L, S, K, roll):
    ops = _ops()
    x = rnd(B, N, L, seed=1)
    w = rnd(M, N, K, seed=2, scale=0.1)
    b = rnd(M, seed=3)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = conv_ref(xd, wd, b.double(), S, roll)
    xg, wg, bg = x.to(DEV), w.to(DEV), b.to(DEV)
    out = ops.conv1d_fwd(ops.Src(xg), wg, bg, S, roll=roll)
    assert out.shape == ref.shape
    assert max_rel(out, ref) < TOL
    da = rnd(*ref.shape, seed=4)
    ref.backward(da.double())
    dag = da.to(DEV)
    dx = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)
    assert max_rel(dx, xd.grad) < TOL
    dw = torch.zeros_like(wg)
    padL = ops.conv_pad(K, S)[0]
    ops.wgrad(ops.Src(dag), ops.Src(xg), dw, K, S, padL, ops.PAD_REFLECT, roll=roll)
    assert max_rel(dw, wd.grad) < TOL
    # accumulation semantics: a second call doubles the gradient
    ops.wgrad(ops.Src(dag), ops.Src(xg), dw, K, S, padL, ops.PAD_REFLECT, roll=roll)
    assert max_rel(dw, 2 * wd.grad) < TOL


def test_conv1d_fwd_dual_source_and_transform():
    """D.enc0-style two pointers + BN/PReLU-on-load (segan_src)."""
    ops = _ops()
    B, L, S, K, M = 3, 256, 4, 31, 20
    x0, x1 = rnd(B, 5, L, seed=1), rnd(B, 3, L, seed=2)
    sc, sh, sl = rnd(8, seed=3), rnd(8, seed=4), rnd(8, seed=5).abs() * 0.3
    w, b = rnd(M, 8, K, seed=6, scale=0.1), rnd(M, seed=7)
    xin = xform_ref(torch.cat((x0, x1), 1), sc, sh, sl)
    ref = conv_ref(xin, w.double(), b.double(), S, roll=-2)
    src = ops.Src(x0.to(DEV), x1.to(DEV), scale=sc.to(DEV), shift=sh.to(DEV), slope=sl.to(DEV))
    out = ops.conv1d_fwd(src, w.to(DEV), b.to(DEV), S, roll=-2)
    assert max_rel(out, ref) < TOL
    # and as the `hi` operand of the weight gradient
    da = rnd(*ref.shape, seed=8)
    wd = w.double().requires_grad_(True)
    conv_ref(xin, wd, None, S, roll=-2).backward(da.double())
    dw = torch.zeros(M, 8, K, device=DEV)
    ops.wgrad(ops.Src(da.to(DEV)), src, dw, K, S, ops.conv_pad(K, S)[0], ops.PAD_REFLECT, roll=-2)
    assert max_rel(dw, wd.grad) < TOL


def test_first_layer_two_pointer_input_with_transform():
    """D.enc0 exactly: x = (clean | noisy) as two one-channel pointers, with a transform, on
    the 1-2 channel VALU kernel."""
    ops = _ops()
    B, L, S, K, M = 3, 2048, 4, 31, 64
    x0, x1 = rnd(B, 1, L, seed=1), rnd(B, 1, L, seed=2)
    sc, sh, sl = rnd(2, seed=3), rnd(2, seed=4), rnd(2, seed=5).abs() * 0.3
    w, b = rnd(M, 2, K, seed=6, scale=0.1), rnd(M, seed=7)
    ref = conv_ref(xform_ref(torch.cat((x0, x1), 1), sc, sh, sl), w.double(), b.double(), S, roll=5)
    src = ops.Src(x0.to(DEV), x1.to(DEV), scale=sc.to(DEV), shift=sh.to(DEV), slope=sl.to(DEV))
    out = ops.conv1d_fwd(src, w.to(DEV), b.to(DEV), S, roll=5)
    assert max_rel(out, ref) < TOL
    out_nb = ops.conv1d_fwd(src, w.to(DEV), None, S, roll=5)
    assert max_rel(out_nb, ref - b.double().view(1, -1, 1)) < TOL


def deconv_ref(x, w, b, S):
    K = w.shape[2]
    pad = max(0, (S - K) // -2)
    y = F.conv_transpose1d(x, w, b, stride=S, padding=pad)
    return y[:, :, :-1] if K % 2 else y


DECONV_CASES = [
    # B, M(Cin), N(Cout), Ls, S, K
    (2, 6, 5, 16, 4, 31),
    (3, 128, 64, 64, 4, 31),
    (2, 16, 1, 256, 4, 31),
    (9, 40, 33, 16, 4, 31),
    (2, 8, 12, 32, 2, 31),
    (1, 24, 130, 1024, 4, 31),
    # stride 2 with few channels: 64-row T tiles with row shifts, 64 / 32-row weight-gradient tiles
    (3, 64, 32, 128, 2, 31),
    (2, 64, 16, 256, 2, 31),
    (2, 32, 8, 64, 2, 31),
    (4, 24, 20, 32, 2, 31),
]


@pytest.mark.parametrize('B,M,N,Ls,S,K', DECONV_CASES)
def test_deconv1d_fwd_dgrad_wgrad(B, M, N, Ls, S, K):
    ops = _ops()
    x = rnd(B, M, Ls, seed=1)
    w = rnd(M, N, K, seed=2, scale=0.1)
    b = rnd(N, seed=3)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = deconv_ref(xd, wd, b.double(), S)
    xg, wg, bg = x.to(DEV), w.to(DEV), b.to(DEV)
    y = ops.deconv1d_fwd(ops.Src(xg), wg, bg, S)
    assert y.shape == ref.shape
    assert max_rel(y, ref) < TOL
    yt = ops.deconv1d_fwd(ops.Src(xg), wg, bg, S, act=ops.ACT_TANH)
    # tanh' <= 1: the output error is bounded by the pre-activation's
    assert (yt.cpu().double() - torch.tanh(ref.detach())).abs().max().item() < \
        max(1e-5, TOL * ref.detach().abs().max().item())
    dy = rnd(*ref.shape, seed=4)
    ref.backward(dy.double())
    dyg = dy.to(DEV)
    _d0, dx = ops.deconv1d_dgrad(dyg, wg, S, 0)
    assert max_rel(dx, xd.grad) < TOL
    if M >= 2:
        M0 = M // 2
        dx0, dx1 = ops.deconv1d_dgrad(dyg, wg, S, M0)
        assert max_rel(dx0, xd.grad[:, :M0]) < TOL
        assert max_rel(dx1, xd.grad[:, M0:]) < TOL
        n0, d1 = ops.deconv1d_dgrad(dyg, wg, S, M0, need0=False)
        assert n0 is None and max_rel(d1, xd.grad[:, M0:]) < TOL
    dw = torch.zeros_like(wg)
    ops.wgrad(ops.Src(xg), ops.Src(dyg), dw, K, S, ops.deconv_pad(K, S), ops.PAD_ZERO)
    assert max_rel(dw, wd.grad) < TOL


def test_deconv1d_skip_concat_alpha_on_load():
    """Decoder input = cat(prelu(prev), alpha * skip) folded into the load
    (generator.py:64-76, 212-222)."""
    ops = _ops()
    B, C, Ls, S, K, N = 3, 24, 64, 4, 31, 10
    prev, skip = rnd(B, C, Ls, seed=1), rnd(B, C, Ls, seed=2)
    s_prev, alpha = rnd(C, seed=3).abs() * 0.2, rnd(C, seed=4)
    w, b = rnd(2 * C, N, K, seed=5, scale=0.1), rnd(N, seed=6)
    ones = torch.ones(C)
    xin = torch.cat((xform_ref(prev, slope=s_prev), xform_ref(skip, scale=alpha)), 1)
    xin.requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = deconv_ref(xin, wd, b.double(), S)
    src = ops.Src(prev.to(DEV), skip.to(DEV), scale=torch.cat((ones, alpha)).to(DEV),
                  slope=torch.cat((s_prev, ones)).to(DEV))
    y = ops.deconv1d_fwd(src, w.to(DEV), b.to(DEV), S)
    assert max_rel(y, ref) < TOL
    dy = rnd(*ref.shape, seed=7)
    ref.backward(dy.double())
    dw = torch.zeros(2 * C, N, K, device=DEV)
    ops.wgrad(src, ops.Src(dy.to(DEV)), dw, K, S, ops.deconv_pad(K, S), ops.PAD_ZERO)
    assert max_rel(dw, wd.grad) < TOL


def test_bn_stats_and_affine_prelu():
    ops = _ops()
    B, C, L = 7, 40, 48
    x = rnd(B, C, L, seed=1) * 3 + 1.5
    gamma, beta, slope = rnd(C, seed=2), rnd(C, seed=3), rnd(C, seed=4).abs() * 0.3
    rm, rv = torch.zeros(C), torch.ones(C)
    ref = F.batch_norm(x.double(), rm.double().clone(), rv.double().clone(), gamma.double(),
                       beta.double(), True, 0.1, 1e-5)
    rm_ref, rv_ref = rm.clone(), rv.clone()
    F.batch_norm(x, rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5)
    rmg, rvg = rm.to(DEV), rv.to(DEV)
    xg = x.to(DEV)
    mean, rstd, scale, shift = ops.bn_stats(xg, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, rmg, rvg)
    assert max_rel(mean, x.double().mean((0, 2))) < 1e-6
    assert max_rel(rmg, rm_ref) < 1e-6 and max_rel(rvg, rv_ref) < 1e-6
    y = ops.affine_prelu(xg, scale, shift, None)
    assert max_rel(y, ref) < 1e-5
    h = ops.affine_prelu(xg, scale, shift, slope.to(DEV))
    assert max_rel(h, F.prelu(ref, slope.double())) < 1e-5


@pytest.mark.parametrize('B,C,L,mu,sd', [(300, 8, 4096, 10.0, 0.1), (300, 64, 16, -3.0, 0.02),
                                         (7, 5, 1001, 0.5, 2.0), (80, 16, 256, 50.0, 1.0)])
def test_bn_stats_one_pass_is_accurate(B, C, L, mu, sd):
    """The BatchNorm statistics are taken in ONE pass (shifted sums per thread, Chan merges): mean
    and variance against fp64 also where the mean is 100 x the spread — the regime in which a
    one-pass variance with a badly chosen shift cancels."""
    ops = _ops()
    x = (rnd(B, C, L, seed=31) * sd + mu + rnd(C, seed=32).view(1, C, 1) * sd).float()
    xd = x.double()
    mean_ref = xd.mean((0, 2))
    var_ref = xd.var((0, 2), unbiased=False)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    mean, rstd, scale, shift = ops.bn_stats(x.to(DEV), None, None, 0.0, 1.0, rm, rv)
    var = 1.0 / (rstd.double().cpu() ** 2)
    assert ((mean.double().cpu() - mean_ref).abs() / var_ref.sqrt()).max().item() < 5e-5   # fp32 data at |mean| = 150 x spread
    assert ((var - var_ref).abs() / var_ref).max().item() < 2e-4
    n = B * L
    assert max_rel(rv, var_ref * n / (n - 1)) < 2e-4      # momentum 1: the unbiased batch variance


@pytest.mark.parametrize('B,C,L', [(6, 24, 32), (300, 8, 16), (3, 70, 1000)])
def test_act_bwd_bn_prelu(B, C, L):
    """Backward through BatchNorm(train) + PReLU incl. gamma/beta/slope/bias grads."""
    ops = _ops()
    c = rnd(B, C, L, seed=1) * 2 + 0.3
    gamma, beta = rnd(C, seed=2) + 1.5, rnd(C, seed=3)
    slope = rnd(C, seed=4).abs() * 0.3
    dh = rnd(B, C, L, seed=5)
    cd = c.double().requires_grad_(True)
    gd, bd, sd = (t.double().requires_grad_(True) for t in (gamma, beta, slope))
    a = F.batch_norm(cd, None, None, gd, bd, True, 0.1, 1e-5)
    F.prelu(a, sd).backward(dh.double())
    cg = c.to(DEV)
    mean, rstd, scale, shift = ops.bn_stats(cg, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, None, None)
    dsl, dga, dbe, dbi = (torch.zeros(C, device=DEV) for _ in range(4))
    dc = ops.act_bwd(cg, dh.to(DEV), slope=slope.to(DEV),
                     bn=(mean, rstd, gamma.to(DEV), beta.to(DEV)),
                     dslope=dsl, dgamma=dga, dbeta=dbe, dbias=dbi)
    assert max_rel(dc, cd.grad) < 2e-5
    assert max_rel(dsl, sd.grad) < 2e-5
    assert max_rel(dga, gd.grad) < 2e-5
    assert max_rel(dbe, bd.grad) < 2e-5
    # a bias in front of BatchNorm has a mathematically zero gradient
    assert dbi.abs().max().item() < 1e-3 * dh.abs().sum().item() / C


def test_act_bwd_prelu_skip():
    """G encoder backward: da = dh*prelu'(a) + alpha*dskip; dslope, dalpha, dbias."""
    ops = _ops()
    B, C, L = 5, 33, 64
    a, dh, dsk = rnd(B, C, L, seed=1), rnd(B, C, L, seed=2), rnd(B, C, L, seed=3)
    slope, alpha = rnd(C, seed=4).abs() * 0.3, rnd(C, seed=5)
    ad = a.double().requires_grad_(True)
    sd, al = slope.double().requires_grad_(True), alpha.double().requires_grad_(True)
    h = F.prelu(ad, sd)
    sk = al.view(1, -1, 1) * ad
    ((h * dh.double()).sum() + (sk * dsk.double()).sum()).backward()
    dsl, dal, dbi = (torch.zeros(C, device=DEV) for _ in range(3))
    da = ops.act_bwd(a.to(DEV), dh.to(DEV), dskip=dsk.to(DEV), slope=slope.to(DEV),
                     alpha=alpha.to(DEV), dslope=dsl, dalpha=dal, dbias=dbi)
    assert max_rel(da, ad.grad) < 1e-5
    assert max_rel(dsl, sd.grad) < 1e-5
    assert max_rel(dal, al.grad) < 1e-5
    assert max_rel(dbi, ad.grad.sum((0, 2))) < 1e-5
    # PReLU initialised at 0 (modules.py:81): slope 0, and a == 0 exactly
    a0 = a.clone()
    a0[0, 0, :5] = 0.0
    z = torch.zeros(C)
    da0 = ops.act_bwd(a0.to(DEV), dh.to(DEV), slope=z.to(DEV))
    want = torch.where(a0 > 0, dh, torch.zeros_like(dh))
    assert max_rel(da0, want) < 1e-6


def test_tanh_bwd_with_l1():
    ops = _ops()
    B, L = 4, 512
    y = torch.tanh(rnd(B, 1, L, seed=1))
    dy, clean = rnd(B, 1, L, seed=2), rnd(B, 1, L, seed=3).clamp(-1, 1)
    db = torch.zeros(1, device=DEV)
    da = ops.tanh_bwd(y.to(DEV), dy.to(DEV), clean=clean.to(DEV), l1_scale=0.25, dbias=db)
    want = (dy.double() + 0.25 * torch.sign(y.double() - clean.double())) * (1 - y.double() ** 2)
    assert max_rel(da, want) < 1e-5
    assert max_rel(db, want.sum().view(1)) < 1e-5
    da2 = ops.tanh_bwd(y.to(DEV), dy.to(DEV))
    assert max_rel(da2, dy.double() * (1 - y.double() ** 2)) < 1e-5


@pytest.mark.parametrize('Bn,I,Oo', [(5, 512, 256), (300, 16384, 256), (7, 256, 128), (3, 128, 1)])
def test_dense_head_gemms(Bn, I, Oo):
    ops = _ops()
    x, w, dy = rnd(Bn, I, seed=1), rnd(Oo, I, seed=2, scale=0.05), rnd(Bn, Oo, seed=3)
    xg, wg, dyg = x.to(DEV), w.to(DEV), dy.to(DEV)
    assert max_rel(ops.linear_fwd(xg, wg), x.double() @ w.double().t()) < TOL
    assert max_rel(ops.linear_dgrad(dyg, wg), dy.double() @ w.double()) < TOL
    dw = torch.zeros_like(wg)
    ops.linear_wgrad(dyg, xg, dw)
    ops.linear_wgrad(dyg, xg, dw)
    assert max_rel(dw, 2 * dy.double().t() @ x.double()) < TOL


def test_bias_prelu_rows_fwd_bwd():
    ops = _ops()
    R, Cc = 9, 256
    x, b, s, dy = rnd(R, Cc, seed=1), rnd(Cc, seed=2), rnd(Cc, seed=3).abs() * 0.3, rnd(R, Cc, seed=4)
    xd = x.double().requires_grad_(True)
    bd, sd = b.double().requires_grad_(True), s.double().requires_grad_(True)
    ref = F.prelu(xd + bd, sd)
    ref.backward(dy.double())
    y = ops.bias_prelu_rows(x.to(DEV), b.to(DEV), s.to(DEV))
    assert max_rel(y, ref) < 1e-6
    ds, db = torch.zeros(Cc, device=DEV), torch.zeros(Cc, device=DEV)
    dx = ops.bias_prelu_rows_bwd(x.to(DEV), b.to(DEV), s.to(DEV), dy.to(DEV), ds, db)
    assert max_rel(dx, xd.grad) < 1e-6 and max_rel(ds, sd.grad) < 1e-5
    assert max_rel(db, bd.grad) < 1e-5


def test_losses():
    ops = _ops()
    from segan_pytorch_amd import losses
    d = rnd(300, seed=1).to(DEV).requires_grad_(True)
    l = losses.MSELoss()(d, 1.0)
    (3.0 * l).backward()
    dd = d.detach().cpu().double().requires_grad_(True)
    lr = F.mse_loss(dd, torch.ones(300, dtype=torch.float64))
    (3.0 * lr).backward()
    assert abs(l.item() - lr.item()) < 1e-6 * max(1, abs(lr.item()))
    assert max_rel(d.grad, dd.grad) < 1e-6
    x = rnd(3, 1, 4096, seed=2).to(DEV).requires_grad_(True)
    y = rnd(3, 1, 4096, seed=3).to(DEV)
    l1 = losses.l1_loss(x, y)
    (100.0 * l1).backward()
    xd = x.detach().cpu().double().requires_grad_(True)
    l1r = F.l1_loss(xd, y.cpu().double())
    (100.0 * l1r).backward()
    assert abs(l1.item() - l1r.item()) < 1e-6
    assert max_rel(x.grad, xd.grad) < 1e-6


def test_fused_optimizers_match_torch():
    from segan_pytorch_amd import optim as soptim
    shapes = [(5, 3, 31), (7,), (1, 6, 1), (130, 4)]
    for kind in ('rmsprop', 'adam'):
        ps = [torch.nn.Parameter(rnd(*s, seed=i)) for i, s in enumerate(shapes)]
        qs = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ps]
        if kind == 'rmsprop':
            ref = torch.optim.RMSprop(ps, lr=5e-5)
            opt = soptim.RMSprop(qs, lr=5e-5)
        else:
            ref = torch.optim.Adam(ps, lr=5e-5, betas=(0.0, 0.9))
            opt = soptim.Adam(qs, lr=5e-5, betas=(0, 0.9))
        for it in range(3):
            for i, (p, q) in enumerate(zip(ps, qs)):
                g = rnd(*p.shape, seed=100 + 10 * it + i)
                p.grad = g.clone()
                q.grad.copy_(g.to(DEV))
            ref.step()
            opt.step()
        for p, q in zip(ps, qs):
            assert (q.detach().cpu() - p.detach()).abs().max().item() < 2e-7, kind
        assert set(opt.state_dict()['state'][0].keys()) == set(ref.state_dict()['state'][0].keys())
        opt.zero_grad()
        assert all(float(q.grad.abs().max()) == 0.0 for q in qs)


def test_cpu_tensor_raises_no_fallback():
    ops = _ops()
    with pytest.raises(RuntimeError):
        ops.Src(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError):
        ops.conv1d_fwd(ops.Src(torch.zeros(1, 1, 64, device=DEV)), torch.zeros(4, 1, 31), None, 4)


def test_bce_logits_const():
    from segan_pytorch_amd import losses
    d = rnd(300, seed=1).to(DEV).requires_grad_(True)
    for target in (1.0, 0.0):
        d.grad = None
        l = losses.BCEWithLogitsLoss()(d, target)
        (0.25 * l).backward()
        dd = d.detach().cpu().double().requires_grad_(True)
        lr = F.binary_cross_entropy_with_logits(dd, torch.full((300,), target, dtype=torch.float64))
        (0.25 * lr).backward()
        assert abs(l.item() - lr.item()) < 1e-6
        assert max_rel(d.grad, dd.grad) < 1e-5


def test_sum_skip():
    ops = _ops()
    x0, x1 = rnd(3, 20, 64, seed=1), rnd(3, 20, 64, seed=2)
    sl, al = rnd(20, seed=3).abs() * 0.3, rnd(20, seed=4)
    out = ops.sum_skip(x0.to(DEV), sl.to(DEV), x1.to(DEV), al.to(DEV))
    want = xform_ref(x0, slope=sl) + al.double().view(1, -1, 1) * x1.double()
    assert max_rel(out, want) < 1e-6


# ---- edge geometry of the contraction kernels -------------------------------------------
EDGE_CONV = [
    # B, N, M, L, S, K, roll : single sample, shortest lengths, odd channel counts, even K
    (1, 5, 7, 32, 4, 31, 0),
    (1, 64, 64, 64, 4, 31, -5),
    (2, 3, 130, 64, 2, 31, 0),
    (300, 4, 8, 32, 4, 31, 1),
    (2, 7, 9, 64, 4, 32, 0),
    (3, 2, 3, 48, 2, 7, 2),
    (2, 512, 40, 64, 4, 31, 0),
    # first-layer VALU kernel (1-2 input channels): > 64 output channels (two weight chunks),
    # strides 2 and 1, short kernels, lengths that are not multiples of the 256-wide tile, 300
    # samples (the weight gradient needs L/S to be a multiple of 4)
    (2, 2, 70, 1200, 4, 31, 3),
    (3, 1, 130, 528, 4, 31, -4),
    (2, 2, 9, 304, 2, 31, 1),
    (2, 1, 5, 100, 1, 31, -2),
    (4, 2, 64, 64, 4, 5, 0),
    (300, 2, 64, 512, 4, 31, 2),
    # long enough for the 4-positions-per-thread edge kernel (L/4 + 8 >= 1024)
    (2, 2, 64, 8192, 4, 31, 3),
    (3, 1, 16, 4112, 4, 31, -7),
    # the same kernel at stride 2 (vanilla11's first layer), with a pitch > 64 (M = 70: runtime-pitch
    # instance), an odd channel count inside a pass of 8, and a short kernel in the 32-tap layout
    (2, 1, 16, 4096, 2, 31, 0),
    (2, 2, 16, 2104, 2, 31, -3),
    (2, 2, 70, 4096, 4, 31, 1),
    (2, 1, 13, 2048, 2, 31, 2),
    (2, 2, 11, 4096, 4, 7, 0),
]


@pytest.mark.parametrize('B,N,M,L,S,K,roll', EDGE_CONV)
def test_conv_edge_geometry(B, N, M, L, S, K, roll):
    test_conv1d_fwd_dgrad_wgrad(B, N, M, L, S, K, roll)


EDGE_DECONV = [
    (1, 5, 7, 8, 4, 31), (1, 3, 2, 16, 4, 31), (300, 4, 6, 8, 4, 31), (2, 130, 3, 16, 2, 31),
    (2, 1024, 24, 16, 4, 31),
    # last-layer shape (1-2 output channels) long enough for the 4-positions-per-thread kernel
    (2, 128, 1, 2048, 4, 31), (3, 20, 2, 1100, 4, 31),
]


@pytest.mark.parametrize('B,M,N,Ls,S,K', EDGE_DECONV)
def test_deconv_edge_geometry(B, M, N, Ls, S, K):
    test_deconv1d_fwd_dgrad_wgrad(B, M, N, Ls, S, K)


def test_unsupported_geometry_reports_error_not_crash():
    ops = _ops()
    x = torch.zeros(1, 2, 12, device=DEV)
    w = torch.zeros(3, 2, 31, device=DEV)
    with pytest.raises(RuntimeError, match='reflect'):      # pad 15 needs L > 15
        ops.conv1d_fwd(ops.Src(x), w, None, 1)
    with pytest.raises(RuntimeError, match='multiple of 4'):
        ops.wgrad(ops.Src(torch.zeros(1, 3, 6, device=DEV)), ops.Src(torch.zeros(1, 2, 24, device=DEV)),
                  torch.zeros(3, 2, 31, device=DEV), 31, 4, 14, ops.PAD_REFLECT)


# ---- bf16 matrix-core modes of the forward / data-gradient contractions -----------------
# bf16x3: every fp32 operand split exactly into 3 bf16 planes, 6 partial products -> the
#         error bound is fp32-class; stated tolerance 5e-5 * max|ref| (fp32 path: 3e-5).
# bf16  : operands rounded to bf16 (8-bit mantissa), fp32 accumulate (BASELINE config 5);
#         stated tolerance 2e-2 * max|ref|.
PREC_TOL = {'bf16x3': 5e-5, 'bf16': 2e-2}
PREC_CASES = [(3, 64, 128, 256, 4, 2), (2, 256, 130, 512, 4, 0), (9, 32, 200, 64, 4, 5),
              (2, 16, 72, 128, 2, -1), (300, 128, 256, 64, 4, 3)]


@pytest.mark.parametrize('prec', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('B,N,M,L,S,roll', PREC_CASES)
def test_conv_bf16_modes(prec, B, N, M, L, S, roll):
    ops = _ops()
    K = 31
    x, w, b = rnd(B, N, L, seed=1), rnd(M, N, K, seed=2, scale=0.1), rnd(M, seed=3)
    sl = rnd(N, seed=9).abs() * 0.3
    xin = xform_ref(x, slope=sl).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = conv_ref(xin, wd, b.double(), S, roll)
    da = rnd(*ref.shape, seed=4)
    ref.backward(da.double())
    tol = PREC_TOL[prec]
    dw = torch.zeros(M, N, K, device=DEV)
    ops.set_precision(prec)
    try:
        out = ops.conv1d_fwd(ops.Src(x.to(DEV), slope=sl.to(DEV)), w.to(DEV), b.to(DEV), S, roll=roll)
        dx = ops.conv1d_dgrad(da.to(DEV), w.to(DEV), L, S, roll=roll)
        ops.wgrad(ops.Src(da.to(DEV)), ops.Src(x.to(DEV), slope=sl.to(DEV)), dw, K, S,
                  ops.conv_pad(K, S)[0], ops.PAD_REFLECT, roll=roll)
        kw = ops.last_wgrad_launch()['kernel']
    finally:
        ops.set_precision('fp32')
    if B == 300:        # a SEGAN+ layer geometry: the bf16 weight-gradient kernel took it
        assert kw == 3, kw
    assert max_rel(out, ref) < tol
    assert max_rel(dw, wd.grad) < tol
    # data gradient w.r.t. the transformed input (dgrad does not apply the transform)
    assert max_rel(dx, xin.grad) < tol


@pytest.mark.parametrize('prec', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('B,M,N,Ls,S', [(3, 128, 64, 64, 4), (9, 40, 33, 16, 4), (2, 64, 48, 32, 2),
                                        (300, 2048, 512, 16, 4)])
def test_deconv_bf16_modes(prec, B, M, N, Ls, S):
    ops = _ops()
    K = 31
    if B * M * Ls > 4e6:      # keep the fp64 CPU reference affordable
        B = 6
    x, w, b = rnd(B, M, Ls, seed=1), rnd(M, N, K, seed=2, scale=0.1), rnd(N, seed=3)
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = deconv_ref(xd, wd, b.double(), S)
    dy = rnd(*ref.shape, seed=4)
    ref.backward(dy.double())
    tol = PREC_TOL[prec]
    dw = torch.zeros(M, N, K, device=DEV)
    ops.set_precision(prec)
    try:
        y = ops.deconv1d_fwd(ops.Src(x.to(DEV)), w.to(DEV), b.to(DEV), S)
        dx0, dx1 = ops.deconv1d_dgrad(dy.to(DEV), w.to(DEV), S, M // 2)
        ops.wgrad(ops.Src(x.to(DEV)), ops.Src(dy.to(DEV)), dw, K, S, ops.deconv_pad(K, S),
                  ops.PAD_ZERO)
    finally:
        ops.set_precision('fp32')
    assert max_rel(y, ref) < tol
    assert max_rel(dw, wd.grad) < tol
    assert max_rel(torch.cat((dx0, dx1), 1), xd.grad) < tol


# ---- STFT power loss (WSEGAN, model.py:640-653) --------------------------------------------
def _pow_db_ref(x, n_fft):
    st = torch.stft(x, n_fft=n_fft, hop_length=160, win_length=320, normalized=True,
                    window=torch.ones(320, dtype=x.dtype), return_complex=True)
    return 10 * torch.log10(st.abs() ** 2 + 10e-20)


@pytest.mark.parametrize('B,T,n_fft', [(3, 16384, 2048), (2, 4096, 2048), (5, 1024, 1024),
                                       (2, 2000, 512)])
def test_stft_pow_l1_matches_torch_stft(B, T, n_fft):
    """Spectrum, loss and waveform gradient against torch.stft in fp64 on the CPU.  Stated
    tolerances: |X| 2e-5 of its max; loss 1e-5 relative; gradient 5e-3 of its max (the dB
    derivative 1/(|X|^2+eps) amplifies fp32 roundoff of the weakest bins; measured 2e-4..1e-3)."""
    from segan_pytorch_amd import losses
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, 1, T, generator=g) * 2 - 1)
    y = (x + 0.3 * torch.randn(B, 1, T, generator=g)).clamp(-1, 1)
    xd = x.double().requires_grad_(True)
    ref = torch.nn.functional.l1_loss(_pow_db_ref(xd.squeeze(1), n_fft),
                                      _pow_db_ref(y.double().squeeze(1), n_fft))
    ref.backward()
    # spectrum
    basis = ops.stft_basis(n_fft, 320, DEV)
    S = ops.stft_spectrum(ops.stft_frames(x.squeeze(1).to(DEV).contiguous(), n_fft, 160, 320), basis)
    st = torch.stft(x.double().squeeze(1), n_fft=n_fft, hop_length=160, win_length=320,
                    normalized=True, window=torch.ones(320, dtype=torch.float64),
                    return_complex=True)            # [B, nbins, NF]
    nb = n_fft // 2 + 1
    NF = 1 + T // 160
    assert S.shape[1] == ops.stft_pitch(n_fft) and S.shape[1] % 4 == 0
    assert float(S[:, 2 * nb:].abs().max()) == 0.0 if S.shape[1] > 2 * nb else True
    Sc = torch.complex(S[:, :nb].double().cpu(), S[:, nb:2 * nb].double().cpu()).view(B, NF, nb)
    assert (Sc.transpose(1, 2) - st).abs().max().item() < 2e-5 * st.abs().max().item()
    # loss and gradient
    xg = x.to(DEV).requires_grad_(True)
    loss = losses.stft_pow_l1(xg, y.to(DEV), n_fft)
    loss.backward()
    assert abs(loss.item() - ref.item()) < 1e-5 * abs(ref.item())
    assert max_rel(xg.grad, xd.grad) < 5e-3


# ---- spectral normalisation ------------------------------------------------------------------
@pytest.mark.parametrize('shape,dim', [((40, 24, 31), 0), ((24, 40, 31), 1), ((256, 4000), 0),
                                       ((128,), 0), ((1024, 512, 31), 0), ((8, 3, 5), 1)])
@pytest.mark.parametrize('power_iteration', [True, False])
def test_snorm_fwd_bwd_matches_torch(shape, dim, power_iteration):
    """ops.snorm_fwd / snorm_bwd against torch.nn.utils.spectral_norm's algorithm in fp64:
    u, v after the power iteration, sigma, the normalised weight, and the gradient folded
    back into weight_orig (u, v constants)."""
    import torch.nn.functional as F
    ops = _ops()
    w = rnd(*shape, seed=1, scale=0.3)
    wm = w.double()
    if dim != 0:
        wm = wm.permute(dim, *[d for d in range(w.dim()) if d != dim])
    wm = wm.reshape(wm.size(0), -1)
    u0 = F.normalize(rnd(wm.size(0), seed=2).double(), dim=0)
    v0 = F.normalize(rnd(wm.size(1), seed=3).double(), dim=0)
    u, v = u0.clone(), v0.clone()
    if power_iteration:
        v = F.normalize(torch.mv(wm.t(), u), dim=0, eps=1e-12)
        u = F.normalize(torch.mv(wm, v), dim=0, eps=1e-12)
    wd = w.double().requires_grad_(True)
    wmd = wd if dim == 0 else wd.permute(dim, *[d for d in range(w.dim()) if d != dim])
    sigma = torch.dot(u, torch.mv(wmd.reshape(wm.shape), v))
    w_sn_ref = wd / sigma
    g = rnd(*shape, seed=4)
    w_sn_ref.backward(g.double())

    ug, vg = u0.float().to(DEV), v0.float().to(DEV)
    w_sn, sig = ops.snorm_fwd(w.to(DEV), ug, vg, dim, power_iteration)
    assert max_rel(ug, u) < 2e-5 and max_rel(vg, v) < 2e-5
    assert abs(sig.item() - sigma.item()) < 2e-5 * abs(sigma.item())
    assert max_rel(w_sn, w_sn_ref) < 2e-5
    dw = torch.full(shape, 0.25, device=DEV)          # accumulates
    ops.snorm_bwd(g.to(DEV), w.to(DEV), ug, vg, sig, dim, dw)
    assert max_rel(dw - 0.25, wd.grad) < 5e-5


@pytest.mark.parametrize('M,N,K', [(300, 256, 16384), (300, 16384, 256), (256, 16384, 300),
                                   (1236, 2052, 320), (1236, 320, 2052), (130, 72, 64),
                                   (64, 64, 16), (300, 128, 256), (37, 50, 100)])
@pytest.mark.parametrize('a_kcontig,b_kcontig', [(True, True), (True, False), (False, True),
                                                 (False, False)])
def test_gemm_layouts(M, N, K, a_kcontig, b_kcontig):
    """segan_gemm with every combination of operand layouts (k-contiguous or row-contiguous):
    the 128x128 float4 kernel where its alignment conditions hold, the generic 64x64 kernel
    otherwise; accumulate and overwrite semantics."""
    ops = _ops()
    A = rnd(M, K, seed=1)
    Bm = rnd(K, N, seed=2)
    ref = A.double() @ Bm.double()
    Ad = (A if a_kcontig else A.t().contiguous()).to(DEV)        # [M,K] or [K,M]
    Bd = (Bm.t().contiguous() if b_kcontig else Bm).to(DEV)       # [N,K] or [K,N]
    sam, sak = (K, 1) if a_kcontig else (1, M)
    sbk, sbn = (1, K) if b_kcontig else (N, 1)
    C = torch.full((M, N), 7.0, device=DEV)
    ops.gemm(Ad, sam, sak, Bd, sbk, sbn, C, M, N, K, True)
    assert max_rel(C, ref) < TOL
    ops.gemm(Ad, sam, sak, Bd, sbk, sbn, C, M, N, K, False)
    assert max_rel(C, 2 * ref) < TOL


def test_split_batchnorm_entry_points_equal_the_fused_ones():
    """The two-call forms used by synchronised BatchNorm (bn_partial + bn_final, and
    act_bwd_bn_reduce + act_bwd_bn_apply) against the fused calls on one rank, and with the
    partials of two half-batches gathered as two 'ranks'."""
    ops = _ops()
    B, C, L = 6, 20, 256
    x = rnd(B, C, L, seed=1).to(DEV) * 1.7 + 0.3
    gamma, beta = (rnd(C, seed=2).abs() + 0.5).to(DEV), rnd(C, seed=3).to(DEV)
    slope = (rnd(C, seed=4).abs() * 0.3).to(DEV)
    rm0, rv0 = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    rm1, rv1 = rm0.clone(), rv0.clone()
    rm2, rv2 = rm0.clone(), rv0.clone()
    fused = ops.bn_stats(x, gamma, beta, 1e-5, 0.1, rm0, rv0)
    split = ops.bn_final(ops.bn_partial(x), gamma, beta, 1e-5, 0.1, rm1, rv1)
    halves = torch.cat((ops.bn_partial(x[:3].contiguous()), ops.bn_partial(x[3:].contiguous())), 0)
    two = ops.bn_final(halves.contiguous(), gamma, beta, 1e-5, 0.1, rm2, rv2)
    for a, b_, c in zip(fused, split, two):
        assert max_rel(b_, a) < 1e-6 and max_rel(c, a) < 1e-5
    assert max_rel(rv1, rv0) < 1e-6 and max_rel(rv2, rv0) < 1e-5 and max_rel(rm2, rm0) < 1e-5
    mean, rstd = fused[0], fused[1]
    bn = (mean, rstd, gamma, beta)
    dh = rnd(B, C, L, seed=5).to(DEV)
    g0 = [torch.zeros(C, device=DEV) for _ in range(4)]
    g1 = [torch.zeros(C, device=DEV) for _ in range(4)]
    ref = ops.act_bwd(x, dh, slope=slope, bn=bn, dslope=g0[0], dgamma=g0[1], dbeta=g0[2], dbias=g0[3])
    totals, ws = ops.act_bwd_bn_reduce(x, dh, slope, bn, g1[0], g1[1], g1[2])
    got = ops.act_bwd_bn_apply(x, dh, slope, bn, totals, B * L, g1[3], ws)
    assert max_rel(got, ref) < 1e-6
    for a, b_ in zip(g0[:3], g1[:3]):
        assert max_rel(b_, a) < 1e-6
    assert (g1[3] - g0[3]).abs().max().item() < 1e-4 * max(1.0, dh.abs().max().item())
    # two "ranks": totals summed over the halves, global count
    h = [(x[:3].contiguous(), dh[:3].contiguous()), (x[3:].contiguous(), dh[3:].contiguous())]
    parts = [ops.act_bwd_bn_reduce(xa, da_, slope, bn) for xa, da_ in h]
    tot = parts[0][0] + parts[1][0]
    da2 = torch.cat([ops.act_bwd_bn_apply(xa, da_, slope, bn, tot, B * L) for xa, da_ in h], 0)
    assert max_rel(da2, ref) < 1e-5


def test_bf16x3_is_as_accurate_as_the_fp32_path():
    """The split-bf16 contractions must not be measurably worse than the exact-fp32 MFMA
    kernels against fp64 (both are bounded by the fp32 accumulation): error within 2x of the
    fp32 path's on forward, data gradient and weight gradient (measured: 1.0x, 0.8x, 1.3x)."""
    ops = _ops()
    B, N, M, L, K, S = 4, 128, 256, 1024, 31, 4
    x, w = rnd(B, N, L, seed=1), rnd(M, N, K, seed=2, scale=0.02)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = conv_ref(xd, wd, None, S, 0)
    da = rnd(*ref.shape, seed=3)
    ref.backward(da.double())
    errs = {}
    for mode in ('fp32', 'bf16x3'):
        ops.set_precision(mode)
        try:
            out = ops.conv1d_fwd(ops.Src(x.to(DEV)), w.to(DEV), None, S)
            dx = ops.conv1d_dgrad(da.to(DEV), w.to(DEV), L, S)
            dw = torch.zeros(M, N, K, device=DEV)
            ops.wgrad(ops.Src(da.to(DEV)), ops.Src(x.to(DEV)), dw, K, S, ops.conv_pad(K, S)[0],
                      ops.PAD_REFLECT)
        finally:
            ops.set_precision('fp32')
        errs[mode] = (max_rel(out, ref), max_rel(dx, xd.grad), max_rel(dw, wd.grad))
    for e3, e32 in zip(errs['bf16x3'], errs['fp32']):
        assert e3 < 2.0 * e32 + 1e-7, errs


# ---------------------------------------------------------------------------------------------
# The real layer shapes at batch sizes where the launches take the code paths of the
# benchmarked configuration (B = 300): strided whole-tile rounds, the stream-K tail with its
# slabs + fixed-order fixup kernel, the dead z-half tiles, the large contraction splits of the
# weight gradients.  Reference: torch fp64 on the CPU.
# ---------------------------------------------------------------------------------------------
SCALE_CONV = [
    # name, N, M, L, roll, B
    ('enc1', 64, 128, 4096, 3, 80),
    ('enc1', 64, 128, 4096, -5, 300),
    ('enc2', 128, 256, 1024, -2, 80),
    ('enc2', 128, 256, 1024, 2, 300),
    ('enc3', 256, 512, 256, 5, 80),
    ('enc3', 256, 512, 256, 0, 300),
    ('enc4', 512, 1024, 64, -4, 80),
    ('enc4', 512, 1024, 64, 1, 300),
]


@pytest.mark.parametrize('name,N,M,L,roll,B', SCALE_CONV)
def test_conv_layers_at_batch_scale(name, N, M, L, roll, B):
    ops = _ops()
    S, K = 4, 31
    x = rnd(B, N, L, seed=11)
    sl = rnd(N, seed=12).abs() * 0.3          # PReLU on load, as the encoders consume it
    w = rnd(M, N, K, seed=13, scale=0.05)
    b = rnd(M, seed=14)
    hd = xform_ref(x, slope=sl).requires_grad_(True)      # the activated input the conv sees
    wd = w.double().requires_grad_(True)
    ref = conv_ref(hd, wd, b.double(), S, roll)
    xg, wg, bg, slg = x.to(DEV), w.to(DEV), b.to(DEV), sl.to(DEV)
    src = ops.Src(xg, slope=slg)
    out = ops.conv1d_fwd(src, wg, bg, S, roll=roll)
    info_f = ops.last_corr_launch()
    assert max_rel(out, ref) < TOL
    assert torch.equal(out, ops.conv1d_fwd(src, wg, bg, S, roll=roll))      # bit-reproducible
    da = rnd(*ref.shape, seed=15)
    ref.backward(da.double())
    dag = da.to(DEV)
    dx = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)        # gradient w.r.t. the activated input
    info_t = ops.last_corr_launch()
    assert max_rel(dx, hd.grad) < TOL
    assert torch.equal(dx, ops.conv1d_dgrad(dag, wg, L, S, roll=roll))
    padL = ops.conv_pad(K, S)[0]
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros_like(wg)
            ops.wgrad(ops.Src(dag), src, dw, K, S, padL, ops.PAD_REFLECT, roll=roll)
            assert max_rel(dw, wd.grad) < TOL, det
            if det:
                dw2 = torch.zeros_like(wg)
                ops.wgrad(ops.Src(dag), src, dw2, K, S, padL, ops.PAD_REFLECT, roll=roll)
                assert torch.equal(dw, dw2)
        finally:
            ops.set_deterministic(False)
    # the launches really took the fast kernel, and at these sizes the stream-K tail
    assert info_f['kernel'] == 2 and info_t['kernel'] == 2
    if B == 300 or name in ('enc3', 'enc4'):
        assert info_f['tiles'] >= 64
    test_conv_layers_at_batch_scale.seen = getattr(test_conv_layers_at_batch_scale, 'seen', [])
    test_conv_layers_at_batch_scale.seen.append((name, B, info_f['streamk'], info_t['streamk']))


def test_stream_k_paths_were_exercised():
    """Of the batch-scale cases above, several must have run the stream-K tail in each form."""
    seen = getattr(test_conv_layers_at_batch_scale, 'seen', [])
    if not seen:
        pytest.skip('batch-scale cases did not run')
    assert sum(1 for s in seen if s[2]) >= 2, seen      # F form
    assert sum(1 for s in seen if s[3]) >= 2, seen      # T form


SCALE_DECONV = [
    # name, M0 (first segment), M1 (second segment), N, Ls, B
    ('dec0', 1024, 1024, 512, 16, 80),
    ('dec0', 1024, 1024, 512, 16, 300),
    ('dec1', 512, 512, 256, 64, 80),
    ('dec1', 512, 512, 256, 64, 300),
    ('dec2', 256, 256, 128, 256, 80),
    ('dec2', 256, 256, 128, 256, 300),
    ('dec3', 128, 128, 64, 1024, 80),
    ('dec3', 128, 128, 64, 1024, 300),
]


@pytest.mark.parametrize('name,M0,M1,N,Ls,B', SCALE_DECONV)
def test_deconv_layers_at_batch_scale(name, M0, M1, N, Ls, B):
    """Decoder layers exactly as the generator runs them: two-pointer input (previous layer |
    alpha-scaled skip) with PReLU / alpha on load, data gradient split at the segment
    boundary (dec0: the z half is not computed), weight gradient with a transformed lo."""
    ops = _ops()
    S, K = 4, 31
    M = M0 + M1
    x0, x1 = rnd(B, M0, Ls, seed=21), rnd(B, M1, Ls, seed=22)
    scale = torch.cat((torch.ones(M0), rnd(M1, seed=23)))           # alpha on the skip half
    slope = torch.cat((rnd(M0, seed=24).abs() * 0.3, torch.ones(M1)))
    w = rnd(M, N, K, seed=25, scale=0.05)
    b = rnd(N, seed=26)
    xin = xform_ref(torch.cat((x0, x1), 1), scale, None, slope).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    pad = ops.deconv_pad(K, S)
    ref = F.conv_transpose1d(xin, wd, b.double(), stride=S, padding=pad)[:, :, :S * Ls]
    src = ops.Src(x0.to(DEV), x1.to(DEV), scale=scale.to(DEV), slope=slope.to(DEV))
    wg = w.to(DEV)
    y = ops.deconv1d_fwd(src, wg, b.to(DEV), S)
    info_t = ops.last_corr_launch()
    assert max_rel(y, ref) < TOL
    assert torch.equal(y, ops.deconv1d_fwd(src, wg, b.to(DEV), S))
    dy = rnd(*ref.shape, seed=27)
    ref.backward(dy.double())
    dyg = dy.to(DEV)
    need0 = name != 'dec0'
    dx0, dx1 = ops.deconv1d_dgrad(dyg, wg, S, M0, need0=need0)
    info_f = ops.last_corr_launch()
    assert max_rel(dx1, xin.grad[:, M0:]) < TOL
    if need0:
        assert max_rel(dx0, xin.grad[:, :M0]) < TOL
    else:
        assert dx0 is None
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros_like(wg)
            ops.wgrad(src, ops.Src(dyg), dw, K, S, pad, ops.PAD_ZERO)
            assert max_rel(dw, wd.grad) < TOL, det
        finally:
            ops.set_deterministic(False)
    assert info_t['kernel'] == 2 and info_f['kernel'] == 2


# the shallow layers of the original 11-layer stride-2 SEGAN shape (train.py:199-205 flags): 16 - 64
# channels, where round 6 added the small-row tiles
SCALE_S2 = [
    # name, N (Cin), M (Cout), L, roll, B
    ('v11.enc1', 16, 32, 8192, 3, 40),
    ('v11.enc2', 32, 32, 4096, -2, 40),
    ('v11.enc3', 32, 64, 2048, 5, 40),
    ('v11.enc4', 64, 64, 1024, -1, 300),
]


@pytest.mark.parametrize('name,N,M,L,roll,B', SCALE_S2)
def test_stride2_conv_layers_take_the_small_row_tiles(name, N, M, L, roll, B):
    """Conv forward / data gradient / weight gradient of the 16 - 64-channel stride-2 layers against
    torch fp64, PReLU on load, both reduction modes, bit-reproducible; and the launch records say
    the small-row tiles ran: F form 32 x 256 for <= 32 output channels, T form 32 rows (16 channels) /
    64 rows (32 channels), W form 32 / 64 rows."""
    ops = _ops()
    S, K = 2, 31
    x = rnd(B, N, L, seed=11)
    sl = rnd(N, seed=12).abs() * 0.3
    w = rnd(M, N, K, seed=13, scale=0.05)
    b = rnd(M, seed=14)
    hd = xform_ref(x, slope=sl).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = conv_ref(hd, wd, b.double(), S, roll)
    xg, wg, bg, slg = x.to(DEV), w.to(DEV), b.to(DEV), sl.to(DEV)
    src = ops.Src(xg, slope=slg)
    out = ops.conv1d_fwd(src, wg, bg, S, roll=roll)
    info_f = ops.last_corr_launch()
    assert max_rel(out, ref) < TOL
    assert torch.equal(out, ops.conv1d_fwd(src, wg, bg, S, roll=roll))
    da = rnd(*ref.shape, seed=15)
    ref.backward(da.double())
    dag = da.to(DEV)
    dx = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)
    info_t = ops.last_corr_launch()
    assert max_rel(dx, hd.grad) < TOL
    assert torch.equal(dx, ops.conv1d_dgrad(dag, wg, L, S, roll=roll))
    padL = ops.conv_pad(K, S)[0]
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros_like(wg)
            ops.wgrad(ops.Src(dag), src, dw, K, S, padL, ops.PAD_REFLECT, roll=roll)
            info_w = ops.last_wgrad_launch()
            assert max_rel(dw, wd.grad) < TOL, det
            if det:
                dw2 = torch.zeros_like(wg)
                ops.wgrad(ops.Src(dag), src, dw2, K, S, padL, ops.PAD_REFLECT, roll=roll)
                assert torch.equal(dw, dw2)
        finally:
            ops.set_deterministic(False)
    assert info_f['kernel'] == 2 and info_t['kernel'] == 2 and info_w['kernel'] == 2
    cols = B * (L // S)
    if M <= 32:
        assert info_f['tiles'] == -(-cols // 256)              # one 32-row tile per 256 columns
    # T form: padded coordinates (L + padL + padR - 1) // S + 1 = (L + 14 + 15 - 1) // 2 + 1 columns
    # per sample, 128 per tile
    tcols = B * ((L + 14 + 15 - 1) // 2 + 1)
    npt = 16 if N <= 16 else 32 if N <= 32 else 64
    assert info_t['tiles'] == -(-N // npt) * -(-tcols // (256 if N <= 16 else 128))     # the 16-channel T tile: 256 columns
    assert info_w['tiles'] == -(-N * S // (128 // 16)) * 1       # one row tile of 32 / 64 rows


@pytest.mark.parametrize('kind,B,M,N,Ls,S,roll', [
    # conv: lo = grad of the pre-activation (plain), hi = the 1 - 2 channel input, reflect padding
    ('conv', 3, 64, 2, 1024, 4, 0),          # D first layer: 2 x 2 MFMA blocks
    ('conv', 3, 64, 1, 1024, 4, 0),          # G first layer
    ('conv', 2, 64, 2, 512, 4, -37),         # rolled input (the discriminator's phase shift)
    ('conv', 3, 16, 1, 2048, 2, 0),          # 11-layer shape: 16 rows of a 32-row block
    ('conv', 2, 16, 2, 2048, 2, 5),
    ('conv', 2, 40, 1, 256, 4, 0),           # rows 40 of 64, few steps per wave
    ('conv', 1, 64, 2, 32, 4, 0),            # one step per sample: every step touches both paddings
    # deconv: lo = the layer input in two segments with PReLU / alpha on load, hi = dy, zero padding
    ('deconv', 2, 128, 1, 1024, 4, 0),       # G last layer: 4 row blocks
    ('deconv', 2, 64, 1, 2048, 2, 0),
    ('deconv', 2, 24, 2, 512, 4, 0),
])
def test_long_edge_weight_gradients_stream(kind, B, M, N, Ls, S, roll):
    """The weight gradient of the long 1 - 2 channel edge layers runs on wgrad_edge_kernel (record
    kind 4: a wave per range of 32-column steps, no barrier in the loop) — against torch fp64, atomics
    and slabs, the latter bit-reproducible; a length that is not a multiple of 32 still takes the
    tiled kernel (kind 1)."""
    ops = _ops()
    K = 31
    if kind == 'conv':
        L = S * Ls
        x = rnd(B, N, L, seed=41)
        w = rnd(M, N, K, seed=42, scale=0.05)
        xd = x.double()
        wd = w.double().requires_grad_(True)
        ref = conv_ref(xd, wd, None, S, roll)
        da = rnd(*ref.shape, seed=43)
        ref.backward(da.double())
        lo, hi = ops.Src(da.to(DEV)), ops.Src(x.to(DEV))
        padL, mode = ops.conv_pad(K, S)[0], ops.PAD_REFLECT
        shape = (M, N, K)
    else:
        M0 = M // 2
        x0, x1 = rnd(B, M0, Ls, seed=44), rnd(B, M - M0, Ls, seed=45)
        scale = torch.cat((torch.ones(M0), rnd(M - M0, seed=46)))
        slope = torch.cat((rnd(M0, seed=47).abs() * 0.3, torch.ones(M - M0)))
        w = rnd(M, N, K, seed=48, scale=0.05)
        xin = xform_ref(torch.cat((x0, x1), 1), scale, None, slope)
        wd = w.double().requires_grad_(True)
        pad = ops.deconv_pad(K, S)
        ref = F.conv_transpose1d(xin, wd, None, stride=S, padding=pad)[:, :, :S * Ls]
        dy = rnd(*ref.shape, seed=49)
        ref.backward(dy.double())
        lo = ops.Src(x0.to(DEV), x1.to(DEV), scale=scale.to(DEV), slope=slope.to(DEV))
        hi = ops.Src(dy.to(DEV))
        padL, mode = pad, ops.PAD_ZERO
        shape = (M, N, K)
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros(shape, device=DEV)
            ops.wgrad(lo, hi, dw, K, S, padL, mode, roll=roll)
            info = ops.last_wgrad_launch()
            assert info['kernel'] == 4, info
            assert max_rel(dw, wd.grad) < TOL, (det, info)
            if det:
                dw2 = torch.zeros(shape, device=DEV)
                ops.wgrad(lo, hi, dw2, K, S, padL, mode, roll=roll)
                assert torch.equal(dw, dw2)
                # accumulates into dw like torch accumulates .grad
                ops.wgrad(lo, hi, dw2, K, S, padL, mode, roll=roll)
                assert max_rel(dw2, 2 * wd.grad) < TOL
        finally:
            ops.set_deterministic(False)


def test_edge_weight_gradient_of_a_ragged_length_takes_the_tiled_kernel():
    ops = _ops()
    B, M, N, Ls, S, K = 2, 64, 2, 300, 4, 31
    x = rnd(B, N, S * Ls, seed=51)
    w = rnd(M, N, K, seed=52, scale=0.05)
    wd = w.double().requires_grad_(True)
    ref = conv_ref(x.double(), wd, None, S, 0)
    da = rnd(*ref.shape, seed=53)
    ref.backward(da.double())
    dw = torch.zeros((M, N, K), device=DEV)
    ops.wgrad(ops.Src(da.to(DEV)), ops.Src(x.to(DEV)), dw, K, S, ops.conv_pad(K, S)[0], ops.PAD_REFLECT)
    assert ops.last_wgrad_launch()['kernel'] == 1
    assert max_rel(dw, wd.grad) < TOL


@pytest.mark.parametrize('name,M0,M1,N,Ls,B', [('v11.dec7', 64, 64, 32, 1024, 40), ('v11.dec8', 32, 32, 32, 2048, 40),
                                               ('v11.dec9', 32, 32, 16, 4096, 40)])
def test_stride2_deconv_layers_take_the_small_row_tiles(name, M0, M1, N, Ls, B):
    """The last MFMA decoder layers of the 11-layer stride-2 shape as the generator runs them
    (two-pointer input, PReLU / alpha on load): forward on 64-row T tiles (32 output channels) or
    32-row tiles (16 channels: both phases inside one MFMA block — the stride-2 transposed conv with
    padding 14 has no row shifts), data gradient on the F form, weight gradient on 64-row tiles."""
    ops = _ops()
    S, K = 2, 31
    M = M0 + M1
    x0, x1 = rnd(B, M0, Ls, seed=21), rnd(B, M1, Ls, seed=22)
    scale = torch.cat((torch.ones(M0), rnd(M1, seed=23)))
    slope = torch.cat((rnd(M0, seed=24).abs() * 0.3, torch.ones(M1)))
    w = rnd(M, N, K, seed=25, scale=0.05)
    b = rnd(N, seed=26)
    xin = xform_ref(torch.cat((x0, x1), 1), scale, None, slope).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    pad = ops.deconv_pad(K, S)
    ref = F.conv_transpose1d(xin, wd, b.double(), stride=S, padding=pad)[:, :, :S * Ls]
    src = ops.Src(x0.to(DEV), x1.to(DEV), scale=scale.to(DEV), slope=slope.to(DEV))
    wg = w.to(DEV)
    y = ops.deconv1d_fwd(src, wg, b.to(DEV), S)
    info_t = ops.last_corr_launch()
    assert max_rel(y, ref) < TOL
    assert torch.equal(y, ops.deconv1d_fwd(src, wg, b.to(DEV), S))
    dy = rnd(*ref.shape, seed=27)
    ref.backward(dy.double())
    dyg = dy.to(DEV)
    dx0, dx1 = ops.deconv1d_dgrad(dyg, wg, S, M0)
    assert max_rel(dx1, xin.grad[:, M0:]) < TOL and max_rel(dx0, xin.grad[:, :M0]) < TOL
    for det in (False, True):
        ops.set_deterministic(det)
        try:
            dw = torch.zeros_like(wg)
            ops.wgrad(src, ops.Src(dyg), dw, K, S, pad, ops.PAD_ZERO)
            info_w = ops.last_wgrad_launch()
            assert max_rel(dw, wd.grad) < TOL, det
        finally:
            ops.set_deterministic(False)
    assert info_t['kernel'] == 2 and info_w['kernel'] == 2
    assert info_t['tiles'] == 1 * -(-(B * Ls) // 256)            # ONE row tile: 32 (or 16) channels x 2 phases, 256 columns
    assert info_w['tiles'] == -(-N * S // 8) * -(-M // (64 if M <= 64 else 128))


@pytest.mark.parametrize('prec', ['bf16x3', 'bf16'])
@pytest.mark.parametrize('name,N,M,L,roll,B', [('enc1', 64, 128, 4096, 3, 80), ('enc2', 128, 256, 1024, -2, 80),
                                               ('enc4', 512, 1024, 64, 1, 300)])
def test_conv_layers_at_batch_scale_bf16(prec, name, N, M, L, roll, B):
    """The bf16 / bf16x3 forms on real layer shapes at batch scale (packed activations, both
    operands by LDS-DMA, slab stream-K tail): forward and data gradient vs fp64 at the restated
    tolerances, and bit-reproducible (no atomics anywhere in these forms)."""
    ops = _ops()
    S, K = 4, 31
    x = rnd(B, N, L, seed=11)
    sl = rnd(N, seed=12).abs() * 0.3
    w = rnd(M, N, K, seed=13, scale=0.05)
    b = rnd(M, seed=14)
    hd = xform_ref(x, slope=sl).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    ref = conv_ref(hd, wd, b.double(), S, roll)
    da = rnd(*ref.shape, seed=15)
    ref.backward(da.double())
    xg, wg, bg, slg, dag = x.to(DEV), w.to(DEV), b.to(DEV), sl.to(DEV), da.to(DEV)
    src = ops.Src(xg, slope=slg)
    ops.set_precision(prec)
    try:
        out = ops.conv1d_fwd(src, wg, bg, S, roll=roll)
        kf = ops.last_corr_launch()['kernel']
        out2 = ops.conv1d_fwd(src, wg, bg, S, roll=roll)
        dx = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)
        kd = ops.last_corr_launch()['kernel']
        dx2 = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)
    finally:
        ops.set_precision('fp32')
    # the bf16 matrix-core kernel (3 = corr_bf2_kernel) took every SEGAN+ layer geometry: an
    # entry point that declines (SEGAN_EUNSUPPORTED) silently runs the fp32 form instead
    assert kf == 3 and kd == 3, (kf, kd)
    tol = PREC_TOL[prec]
    assert max_rel(out, ref) < tol and max_rel(dx, hd.grad) < tol
    assert torch.equal(out, out2) and torch.equal(dx, dx2)


@pytest.mark.parametrize('prec,name,M0,M1,N,Ls,B', [
    (p, *c) for p in ('bf16x3', 'bf16')
    for c in (('dec0', 1024, 1024, 512, 16, 300 if p == 'bf16' or os.environ.get('SEGAN_TEST_FULL') == '1' else 80),
              ('dec2', 256, 256, 128, 256, 80), ('dec3', 128, 128, 64, 1024, 80))])
def test_deconv_layers_at_batch_scale_bf16(prec, name, M0, M1, N, Ls, B):
    """Decoder layers in the bf16 / bf16x3 forms at batch scale: two-pointer input with alpha /
    PReLU applied by the packing pass, data gradient split at the segment boundary."""
    ops = _ops()
    S, K = 4, 31
    M = M0 + M1
    x0, x1 = rnd(B, M0, Ls, seed=21), rnd(B, M1, Ls, seed=22)
    scale = torch.cat((torch.ones(M0), rnd(M1, seed=23)))
    slope = torch.cat((rnd(M0, seed=24).abs() * 0.3, torch.ones(M1)))
    w = rnd(M, N, K, seed=25, scale=0.05)
    b = rnd(N, seed=26)
    xin = xform_ref(torch.cat((x0, x1), 1), scale, None, slope).requires_grad_(True)
    wd = w.double().requires_grad_(True)
    pad = ops.deconv_pad(K, S)
    ref = F.conv_transpose1d(xin, wd, b.double(), stride=S, padding=pad)[:, :, :S * Ls]
    dy = rnd(*ref.shape, seed=27)
    ref.backward(dy.double())
    src = ops.Src(x0.to(DEV), x1.to(DEV), scale=scale.to(DEV), slope=slope.to(DEV))
    wg, bg, dyg = w.to(DEV), b.to(DEV), dy.to(DEV)
    need0 = name != 'dec0'
    ops.set_precision(prec)
    try:
        y = ops.deconv1d_fwd(src, wg, bg, S)
        kf = ops.last_corr_launch()['kernel']
        y2 = ops.deconv1d_fwd(src, wg, bg, S)
        dx0, dx1 = ops.deconv1d_dgrad(dyg, wg, S, M0, need0=need0)
        kd = ops.last_corr_launch()['kernel']
        dx0b, dx1b = ops.deconv1d_dgrad(dyg, wg, S, M0, need0=need0)
    finally:
        ops.set_precision('fp32')
    assert kf == 3 and kd == 3, (kf, kd)         # corr_bf2_kernel, not the fp32 fall-back
    tol = PREC_TOL[prec]
    assert max_rel(y, ref) < tol and torch.equal(y, y2)
    assert max_rel(dx1, xin.grad[:, M0:]) < tol and torch.equal(dx1, dx1b)
    if need0:
        assert max_rel(dx0, xin.grad[:, :M0]) < tol
    else:
        assert dx0 is None


# One tile epilogue serves the fp32 and the bf16 kernels.  Its fast stores (buffer stores per row,
# 16-byte quad stores at stride 4, 8-byte pair stores at stride 2 in fp32) are taken only by tiles
# whose rows are all real channels; one channel fewer and the same tile takes the generic
# per-element form.  Each case is run with C and with C - 1 channels (the last slice of the same
# weight and bias dropped): same kernel, same tile plan, and the common channels are the same bits.
EPILOGUE_CASES = [
    # op, sizes (B = 2, K = 31); `drop` names the dimension that loses its last channel
    ('deconv_fwd', dict(M=32, N=32, Ls=128, S=4)),                   # quad
    ('deconv_fwd', dict(M=32, N=64, Ls=128, S=2)),                   # pair (fp32), 128-row tile
    ('deconv_fwd', dict(M=32, N=32, Ls=128, S=2)),                   # pair (fp32), 64-row tile
    ('deconv_fwd', dict(M=32, N=16, Ls=128, S=2)),                   # pair (fp32), 32-row tile
    ('conv_dgrad', dict(M=40, N=32, L=1024, S=4, roll=-3)),          # quad with halo and roll
    ('conv_dgrad', dict(M=40, N=64, L=1024, S=4, roll=2)),
    ('conv_fwd', dict(M=128, N=16, L=512, S=4)),                     # F form interior buffer stores
    ('deconv_dgrad', dict(M=128, N=16, Ls=128, S=4, M0=64)),         # two destinations
]
_epilogue_refs = {}


def _epilogue_inputs(op, g):
    """fp32 inputs of a case and its fp64 outputs (computed once, shared by the precisions)."""
    key = (op, tuple(sorted(g.items())))
    if key not in _epilogue_refs:
        B, K, S, M, N = 2, 31, g['S'], g['M'], g['N']
        if op == 'deconv_fwd':
            x, w, b = rnd(B, M, g['Ls'], seed=31), rnd(M, N, K, seed=32, scale=0.1), rnd(N, seed=33)
            ref = [deconv_ref(x.double(), w.double(), b.double(), S)]
        elif op == 'conv_dgrad':
            x, w, b = rnd(B, M, g['L'] // S, seed=31), rnd(M, N, K, seed=32, scale=0.1), None
            x0 = torch.zeros(B, N, g['L'], dtype=torch.float64, requires_grad=True)
            conv_ref(x0, w.double(), None, S, g['roll']).backward(x.double())
            ref = [x0.grad]
        elif op == 'conv_fwd':
            x, w, b = rnd(B, N, g['L'], seed=31), rnd(M, N, K, seed=32, scale=0.1), rnd(M, seed=33)
            ref = [conv_ref(x.double(), w.double(), b.double(), S)]
        else:
            x, w, b = rnd(B, N, S * g['Ls'], seed=31), rnd(M, N, K, seed=32, scale=0.1), None
            x0 = torch.zeros(B, M, g['Ls'], dtype=torch.float64, requires_grad=True)
            deconv_ref(x0, w.double(), None, S).backward(x.double())
            ref = [x0.grad[:, :g['M0']], x0.grad[:, g['M0']:]]
        _epilogue_refs[key] = (x, w, b, ref)
    return _epilogue_refs[key]


def _epilogue_run(ops, op, g, x, w, b, drop):
    """The op with the last `drop` (0 / 1) channels of its output dimension left out."""
    xg = x.to(DEV)
    if op == 'deconv_fwd':
        n = g['N'] - drop
        out = [ops.deconv1d_fwd(ops.Src(xg), w[:, :n].contiguous().to(DEV), b[:n].to(DEV), g['S'])]
    elif op == 'conv_dgrad':
        n = g['N'] - drop
        out = [ops.conv1d_dgrad(xg, w[:, :n].contiguous().to(DEV), g['L'], g['S'], roll=g['roll'])]
    elif op == 'conv_fwd':
        m = g['M'] - drop
        out = [ops.conv1d_fwd(ops.Src(xg), w[:m].to(DEV), b[:m].to(DEV), g['S'])]
    else:
        m = g['M'] - drop
        out = list(ops.deconv1d_dgrad(xg, w[:m].to(DEV), g['S'], g['M0']))
    return out, ops.last_corr_launch()


@pytest.mark.parametrize('prec', ['fp32', 'bf16x3', 'bf16'])
def test_fast_and_generic_epilogues_store_the_same_bits(prec):
    ops = _ops()
    tol = TOL if prec == 'fp32' else PREC_TOL[prec]
    for op, g in EPILOGUE_CASES:
        x, w, b, ref = _epilogue_inputs(op, g)
        ops.set_precision(prec)
        try:
            full, info_full = _epilogue_run(ops, op, g, x, w, b, 0)
            less, info_less = _epilogue_run(ops, op, g, x, w, b, 1)
        finally:
            ops.set_precision('fp32')
        what = (op, g)
        # 3 = corr_bf2_kernel: an entry point that declines silently runs the fp32 form instead
        assert info_full['kernel'] == (2 if prec == 'fp32' else 3), what
        assert (info_full['kernel'], info_full['tiles']) == (info_less['kernel'], info_less['tiles']), what
        for f, r in zip(full, ref):
            assert f.shape == r.shape and max_rel(f, r) < tol, what
        # the last tensor is the one that lost a channel; the others are whole
        for f, s in zip(full[:-1], less[:-1]):
            assert torch.equal(f, s), what
        c = less[-1].shape[1]
        assert c == full[-1].shape[1] - 1 and torch.equal(full[-1][:, :c], less[-1]), what


def test_stream_k_fixup_is_order_fixed_bf16():
    """bf16 enc3 at B = 80: the cut tiles of the stream-K tail are summed by the fix-up kernel the
    fp32 kernels use, slabs in chunk order — forward and data gradient are the same bits twice."""
    ops = _ops()
    name, N, M, L, roll, B = next(c for c in SCALE_CONV if c[0] == 'enc3' and c[5] == 80)
    S, K = 4, 31
    xg, slg = rnd(B, N, L, seed=11).to(DEV), (rnd(N, seed=12).abs() * 0.3).to(DEV)
    wg, bg = rnd(M, N, K, seed=13, scale=0.05).to(DEV), rnd(M, seed=14).to(DEV)
    dag = rnd(B, M, L // S, seed=15).to(DEV)
    src = ops.Src(xg, slope=slg)
    ops.set_precision('bf16')
    try:
        out = ops.conv1d_fwd(src, wg, bg, S, roll=roll)
        info_f = ops.last_corr_launch()
        out2 = ops.conv1d_fwd(src, wg, bg, S, roll=roll)
        dx = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)
        info_t = ops.last_corr_launch()
        dx2 = ops.conv1d_dgrad(dag, wg, L, S, roll=roll)
    finally:
        ops.set_precision('fp32')
    assert info_f['kernel'] == 3 and info_t['kernel'] == 3, (info_f, info_t)
    assert info_f['streamk'] or info_t['streamk'], (info_f, info_t)
    assert torch.equal(out, out2) and torch.equal(dx, dx2)


def l2_rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize('gated', [False, True])
def test_discriminator_batchnorm_at_batch_300(gated):
    """One D forward + backward with BatchNorm statistics over 300 x L samples per channel
    against the CPU oracle (segan_oracle.discriminator_forward, fp32): logits, every parameter
    gradient, and the running statistics.

    gated=False: PReLU slopes 1 (identity) — the BatchNorm / conv / dense chain alone, strict.
    gated=True: slopes 0.05..0.3.  A PReLU gate is discontinuous in its derivative: of the
    ~10^7 pre-activations a handful sit within fp32 roundoff of zero, the CPU and the GPU take
    different sides there, and each such flip moves the gradients downstream by a discrete
    amount (measured vs an fp64 oracle, test_discriminator_gradients_with_aligned_gates: GPU 2e-3, fp32 CPU oracle
    2e-4..6e-4 in relative L2; the forward agrees to 4e-6).  Bound: 6e-3 relative L2."""
    from segan_pytorch_amd.models import Discriminator
    from segan_pytorch_amd import losses
    B = 300
    torch.manual_seed(5)
    D = Discriminator(2, [64, 128, 256, 512, 1024], 31, poolings=[4] * 5, pool_type='none',
                      pool_slen=16, norm_type='bnorm', phase_shift=5)
    for n_, p in D.named_parameters():       # leave the symmetric initial point
        if n_.endswith('act.weight'):
            if gated:
                p.data.uniform_(0.05, 0.3)
            else:
                p.data.fill_(1.0)
        elif n_.endswith('conv.weight'):
            p.data.normal_(0.0, 0.02)
    sd0 = {k: v.detach().clone() for k, v in D.state_dict().items()}
    D = D.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 2, 16384, generator=g) * 2 - 1
    rolls = [2, -5, 1, -1, 4]
    D.draw_rolls = lambda: list(rolls)
    y, _ = D(x[:, :1].contiguous().to(DEV), x[:, 1:].contiguous().to(DEV))
    loss = losses.MSELoss()(y.view(-1), 1.0)
    loss.backward()
    torch.cuda.synchronize()
    sd = {k: (v.clone().requires_grad_(True) if torch.is_floating_point(v) and
              k.split('.')[-1] not in O._BUFFERS else v.clone()) for k, v in sd0.items()}
    yo = O.discriminator_forward(sd, x, rolls, [4] * 5)
    lo = F.mse_loss(yo.view(-1), torch.ones(B))
    keys = [k for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad]
    grads = torch.autograd.grad(lo, [sd[k] for k in keys])
    assert max_rel(y, yo) < 5e-5
    assert max_rel(loss, lo) < 2e-5
    dn = dict(D.named_parameters())
    for k, gr in zip(keys, grads):
        if k.endswith('conv.bias'):
            continue            # zero gradient in front of BatchNorm: roundoff on both sides
        if gr.abs().max().item() < 1e-7:
            # mathematically zero (identity activations: a BatchNorm bias in front of another
            # conv + BatchNorm is cancelled like a conv bias): roundoff on both sides
            assert dn[k].grad.abs().max().item() < 1e-6, k
            continue
        assert l2_rel(dn[k].grad, gr) < (6e-3 if gated else 2e-4), k
    got = D.state_dict()
    for k in sd0:
        if k.endswith('running_mean') or k.endswith('running_var'):
            assert max_rel(got[k], sd[k]) < 2e-5, k


def gpu_discriminator_gates(D):
    """The side of zero every PReLU input of D's LAST forward fell on, on the GPU: the conv
    stack's gates are fmaf(c, scale, shift) > 0 with the BatchNorm (scale, shift) of that forward
    (bit for bit what the consuming kernels and act_bwd_kernel evaluate), the dense head's are
    (y + bias) > 0.  Keys as oracle.discriminator_forward(gates=) takes them."""
    from segan_pytorch_amd import ops
    cs, xfs = D._last_fwd
    gates = {}
    for l, c in enumerate(cs):
        v = c if xfs[l][0] is None else ops.affine_prelu(c, xfs[l][0], xfs[l][1], None)
        gates['h_{}'.format(l)] = (v > 0).cpu()
    hf, y1, a1, y2, a2, y3 = D._last_head
    gates['fc_1'] = ((y1 + D.fc[0].bias.detach()) > 0).cpu()
    gates['fc_3'] = ((y2 + D.fc[2].bias.detach()) > 0).cpu()
    return gates


def discriminator_aligned_gates_run(slopes, precision='fp32', B=300):
    """One D forward + backward at batch B on the GPU in the given contraction precision against an
    fp64 evaluation of the oracle, free-running and with the GPU's PReLU sides imposed (oracle
    `gates=`: where(gate, a, slope*a)).  Returns the figures the two tests below assert:
    flips / total gates, the largest fp64 |a| at a flipped gate, the logits' distance, the
    free-running and the aligned gradient distance (relative L2, worst tensor, with its name)."""
    from segan_pytorch_amd.models import Discriminator
    from segan_pytorch_amd import losses, ops
    torch.manual_seed(5)
    D = Discriminator(2, [64, 128, 256, 512, 1024], 31, poolings=[4] * 5, pool_type='none',
                      pool_slen=16, norm_type='bnorm', phase_shift=5)
    for n_, p in D.named_parameters():
        if n_.endswith('act.weight'):
            if slopes == 'trained':
                p.data.uniform_(0.05, 0.3)
        elif n_.endswith('conv.weight'):
            p.data.normal_(0.0, 0.02)
    sd0 = {k: v.detach().clone() for k, v in D.state_dict().items()}
    D = D.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 2, 16384, generator=g) * 2 - 1
    rolls = [2, -5, 1, -1, 4]
    D.draw_rolls = lambda: list(rolls)
    old, oldp = ops.get_deterministic(), ops.get_precision()
    ops.set_deterministic(True)
    ops.set_precision(precision)
    try:
        y, _ = D(x[:, :1].contiguous().to(DEV), x[:, 1:].contiguous().to(DEV))
        loss = losses.MSELoss()(y.view(-1), 1.0)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(old)
        ops.set_precision(oldp)
    gates = gpu_discriminator_gates(D)
    dn = dict(D.named_parameters())

    def oracle64(gates_):
        sd = {k: (v.double().requires_grad_(True) if torch.is_floating_point(v) and
                  k.split('.')[-1] not in O._BUFFERS else
                  (v.double() if torch.is_floating_point(v) else v.clone())) for k, v in sd0.items()}
        yo, acts = O.discriminator_forward(sd, x.double(), rolls, [4] * 5, ret_act=True, gates=gates_)
        lo = F.mse_loss(yo.view(-1), torch.ones(B, dtype=torch.float64))
        keys = [k for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad]
        return yo, acts, dict(zip(keys, torch.autograd.grad(lo, [sd[k] for k in keys])))

    # (1) the free-running fp64 oracle: where do the sides differ, and how close to zero is that
    y64, acts64, g64 = oracle64(None)
    flips = total = 0
    worst = 0.0
    per_layer = {}
    for k, gate in gates.items():
        a = acts64['a_' + k[2:]] if k.startswith('h_') else acts64['fc_a' + k[3:]]
        diff = gate != (a > 0)
        flips += int(diff.sum())
        total += gate.numel()
        per_layer[k] = int(diff.sum()) / gate.numel()
        if diff.any():
            worst = max(worst, float(a[diff].abs().max()))
    free = max(l2_rel(dn[k].grad, v) for k, v in g64.items()
               if not k.endswith('conv.bias') and v.abs().max().item() >= 1e-7)
    # (2) the same oracle with the GPU's sides
    _, _, g64a = oracle64(gates)
    aligned, worst_key, zero_ok = 0.0, None, True
    for k, gr in g64a.items():
        if k.endswith('conv.bias'):
            continue            # zero gradient in front of BatchNorm: roundoff on both sides
        if gr.abs().max().item() < 1e-7:
            zero_ok = zero_ok and dn[k].grad.abs().max().item() < 1e-6
            continue
        e = l2_rel(dn[k].grad, gr)
        if e > aligned:
            aligned, worst_key = e, k
    out = dict(precision=precision, slopes=slopes, flips=flips, total=total, flip_share=flips / total,
               flip_share_per_layer=per_layer, worst_abs_a_at_a_flip=worst, logits_max_rel=max_rel(y, y64),
               free_running=free, aligned=aligned, aligned_worst_tensor=worst_key, zero_grads_ok=zero_ok)
    print(out)
    return out


# the trained-slopes flavour repeats the two fp64 oracle evaluations at batch 300 (~55 s of host time):
# with SEGAN_TEST_FULL=1 (the GPU suite is budgeted against the driver's 20-minute limit)
@pytest.mark.parametrize('slopes', ['init'] + (['trained'] if os.environ.get('SEGAN_TEST_FULL') == '1' else []))
def test_discriminator_gradients_with_aligned_gates(slopes):
    """What test_discriminator_batchnorm_at_batch_300's 6e-3 allowance rests on, as a test
    (round-3 review, weak point 1; formerly the diagnostics diag_d300.py + diag_gateflips.py).

    One D forward + backward at B = 300 on the GPU against an fp64 evaluation of the oracle:
      (1) the pre-activations on which the two disagree about the PReLU side are COUNTED: they
          must be a vanishing share of the ~4e8 gates, and every one of them must be a value the
          fp64 run holds to be within forward roundoff of zero (|a| < 2e-5 on BatchNorm-normalised,
          i.e. unit-scale, values) — flips happen only where the side is undecidable in fp32;
      (2) with the GPU's sides imposed on the fp64 oracle (oracle `gates=`: where(gate, a,
          slope*a) — the forward value moves by a roundoff, the derivative discontinuity is
          removed) every parameter gradient agrees to 5e-5 relative L2 (measured 5e-6; the
          identity-activation variant is held to 2e-4), i.e. ALL of the free-running gradient
          distance (measured 1.5e-3 .. 1.7e-3 here, 24-26 flipped gates of 1.5e8, none with
          |a| > 5e-6) is those gates.
    slopes = 'init': PReLU slopes 0 in the conv stack and 0.25 in the head, the state the
    benchmarked step runs from (model.py:28-43); 'trained': slopes 0.05..0.3."""
    r = discriminator_aligned_gates_run(slopes, 'fp32')
    assert r['logits_max_rel'] < 5e-5
    assert r['flips'] <= 2e-5 * r['total'], (r['flips'], r['total'])
    assert r['worst_abs_a_at_a_flip'] < 2e-5
    assert r['zero_grads_ok']
    assert r['aligned'] < 5e-5, (r['aligned_worst_tensor'], r['aligned'])


@pytest.mark.parametrize('S', [4, 2, 1])
@pytest.mark.parametrize('M,N,K', [(128, 64, 31), (96, 6, 31), (40, 5, 31), (64, 8, 32), (64, 8, 11), (16, 2, 31)])
def test_packed_f_buffer_is_what_layout_py_states(S, M, N, K):
    """segan_pack_weights' F buffer against layout.pack_f — including the K = 31 channel pairing
    (an even channel count > 2: the padding-tap row of every odd channel holds row 30 of its even
    partner) and the cases that must NOT pair (odd count, two channels, K != 31): bit for bit,
    padding rows / columns zero."""
    from segan_pytorch_amd import layout as lay
    o = _ops()
    w = rnd(M, N, K, seed=S + M)
    buf = o.WeightPack().f(w.to(DEV), S).cpu()
    rows = -(-N * 32 // 64) * 64
    pitch = 64 if M <= 64 else -(-M // 128) * 128
    assert buf.numel() == rows * pitch
    got = buf.view(rows, pitch)
    want = torch.from_numpy(lay.pack_f(w.numpy(), S)).reshape(N * 32, M)        # [(n, r, u), m]
    assert torch.equal(got[:N * 32, :M], want)
    assert float(got[N * 32:].abs().max()) == 0.0 if rows > N * 32 else True
    assert float(got[:, M:].abs().max()) == 0.0 if pitch > M else True
    assert lay.f_pair(N, K) == (K == 31 and N > 2 and N % 2 == 0)


def test_release_scratch_frees_and_the_next_call_reallocates():
    """ops.release_scratch (round-4 advice): the per-stream scratch buffers are handed back, also
    those of a side stream whose torch.cuda.Stream object is gone, and the next contraction call
    allocates what it needs again with the same results."""
    from segan_pytorch_amd import ops
    o = _ops()
    x, w = rnd(4, 64, 1024, seed=1), rnd(128, 64, 31, seed=2, scale=0.05)
    src = o.Src(x.to(DEV))
    y0 = o.conv1d_fwd(src, w.to(DEV), None, 4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y1 = o.conv1d_fwd(src, w.to(DEV), None, 4)
    torch.cuda.synchronize()
    del side
    assert ops.scratch_bytes() >= 2 * (128 << 20)        # one stream-K buffer per stream
    ops.release_scratch()
    assert ops.scratch_bytes() == 0
    y2 = o.conv1d_fwd(src, w.to(DEV), None, 4)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1) and torch.equal(y0, y2)
    assert ops.scratch_bytes() >= (128 << 20)


def test_mse_between_tensors_matches_torch():
    """--reg_loss mse_loss (train.py:179): F.mse_loss(Genh, clean) forward and gradient."""
    from segan_pytorch_amd import losses
    x = rnd(5, 1, 4096, seed=1)
    y = rnd(5, 1, 4096, seed=2)
    xd = x.double().requires_grad_(True)
    ref = F.mse_loss(xd, y.double())
    (3.0 * ref).backward()
    xg = x.to(DEV).requires_grad_(True)
    got = losses.mse_loss(xg, y.to(DEV))
    (3.0 * got).backward()
    assert max_rel(got, ref) < 1e-5
    assert max_rel(xg.grad, xd.grad) < 1e-5


@pytest.mark.parametrize('L', [1, 16, 100])
def test_global_pooling_over_time(L):
    """segan_pool_time_fwd / bwd against torch's AdaptiveMaxPool1d(1) / AdaptiveAvgPool1d(1)
    (the 'gmax' / 'gavg' heads, discriminator.py:128-137), ties included."""
    from segan_pytorch_amd import ops
    torch.manual_seed(L)
    x = torch.randn(5, 7, L)
    if L > 2:
        x[0, 0, 1] = x[0, 0, 2] = 9.0            # a tie: the first position gets the gradient
    dy = torch.randn(5, 7)
    for mode, pool in (('max', torch.nn.AdaptiveMaxPool1d(1)), ('avg', torch.nn.AdaptiveAvgPool1d(1))):
        xr = x.clone().requires_grad_(True)
        yr = pool(xr).squeeze(2)
        yr.backward(dy)
        y, idx = ops.pool_time_fwd(x.to(DEV), mode)
        dx = ops.pool_time_bwd(dy.to(DEV), idx, L, mode)
        assert torch.equal(y.cpu(), yr.detach()) or max_rel(y, yr.detach()) < 1e-6
        assert max_rel(dx, xr.grad) < 1e-6, mode


@pytest.mark.parametrize('B,N,M,L,S,K,roll', [
    (3, 8, 16, 64, 4, 31, 0),        # Ls 16, one partial column tile
    (17, 16, 64, 64, 4, 31, 1),      # three column tiles, the last one partial; rolled
    (9, 4, 32, 128, 4, 31, -3),      # Ls 32
    (5, 12, 48, 64, 4, 5, 2),        # narrow kernel: padL 1, no reachable right halo
    (2, 8, 16, 256, 4, 31, 7),       # Ls 64
    (80, 512, 1024, 64, 4, 31, 0),   # the enc4 shape of the SEGAN+ nets
    (19, 8, 16, 16, 2, 31, 0),       # stride 2, Ls 8: the deepest layer of the 11-layer SEGAN
    (5, 16, 32, 32, 2, 31, -2),      # stride 2, Ls 16
    (3, 4, 16, 128, 2, 31, 3),       # stride 2, Ls 64
    (8, 256, 512, 32, 2, 31, 1),     # a deep layer of the 11-layer net
    (4, 8, 16, 32, 1, 31, 2),        # stride 1 (pooling-1 layers)
    (40, 4, 16, 16, 4, 31, 0),       # Ls 4: 32 samples per column tile
])
def test_conv1d_dgrad_short_rows(B, N, M, L, S, K, roll):
    """segan_conv1d_dgrad_short (GEMM + col2im form, fold and roll in the epilogue) against the
    fp64 autograd of the reflect-padded strided conv, and bit-reproducible."""
    ops = _ops()
    w = rnd(M, N, K, seed=2, scale=0.1)
    da = rnd(B, M, L // S, seed=4)
    xd = torch.zeros(B, N, L, dtype=torch.float64, requires_grad=True)
    conv_ref(xd, w.double(), None, S, roll).backward(da.double())
    dag, wg = da.to(DEV), w.to(DEV)
    dx = ops.conv1d_dgrad_short(dag, wg, L, S, roll=roll)
    assert max_rel(dx, xd.grad) < TOL
    assert torch.equal(dx, ops.conv1d_dgrad_short(dag, wg, L, S, roll=roll))
    if ops.short_rows_ok(N, M, L, S):
        assert torch.equal(dx, ops.conv1d_dgrad(dag, wg, L, S, roll=roll))   # the routed path


@pytest.mark.parametrize('name', ['enc4', 'dec0'])
def test_blocked_accumulation_is_more_accurate(name):
    """ops.set_accumulation('blocked') (SEGAN_PREC_FP32_BLOCKED): forward and data gradient of the
    longest contractions (K = 15 872 / 16 384 terms) against fp64.  Plain accumulation leaves a
    relative L2 error of ~2e-6, blocked ~3e-7 (tests/diag/diag_accum.py); both bit-reproducible."""
    ops = _ops()
    S, K, B = 4, 31, 24

    def l2(a, b):
        a, b = a.double().cpu(), b.double()
        return ((a - b).norm() / b.norm()).item()

    if name == 'enc4':
        N, M, L = 512, 1024, 64
        x, w, b = rnd(B, N, L, seed=1), rnd(M, N, K, seed=2, scale=0.05), rnd(M, seed=3)
        xd = x.double().requires_grad_(True)
        ref = conv_ref(xd, w.double(), b.double(), S)
        da = rnd(*ref.shape, seed=4)
        ref.backward(da.double())
        xg, wg, bg, dag = x.to(DEV), w.to(DEV), b.to(DEV), da.to(DEV)
        run = lambda: (ops.conv1d_fwd(ops.Src(xg), wg, bg, S), ops.conv1d_dgrad(dag, wg, L, S))
        want = (ref.detach(), xd.grad)
    else:
        M, N, Ls = 2048, 512, 16
        x, w, b = rnd(B, M, Ls, seed=5), rnd(M, N, K, seed=6, scale=0.05), rnd(N, seed=7)
        pad = ops.deconv_pad(K, S)
        xd = x.double().requires_grad_(True)
        ref = F.conv_transpose1d(xd, w.double(), b.double(), stride=S, padding=pad)[:, :, :S * Ls]
        dy = rnd(*ref.shape, seed=8)
        ref.backward(dy.double())
        xg, wg, bg, dyg = x.to(DEV), w.to(DEV), b.to(DEV), dy.to(DEV)
        run = lambda: (ops.deconv1d_fwd(ops.Src(xg), wg, bg, S), ops.deconv1d_dgrad(dyg, wg, S, 0)[1])
        want = (ref.detach(), xd.grad)
    errs = {}
    for mode in ('plain', 'blocked'):
        ops.set_accumulation(mode)
        try:
            got = run()
            again = run()
        finally:
            ops.set_accumulation('plain')
        assert all(torch.equal(a, b) for a, b in zip(got, again)), mode
        errs[mode] = [l2(g, r) for g, r in zip(got, want)]
    # forward (both layers) and the deconv data gradient contract over K >= 15 872 terms; the conv
    # data gradient of enc4 runs the short-row GEMM path (K = 1024 per tap), which does not block
    assert errs['blocked'][0] < 6e-7 and errs['blocked'][0] < 0.5 * errs['plain'][0], errs
    assert errs['blocked'][1] < 8e-7, errs
    if name == 'dec0':
        assert errs['blocked'][1] < 0.5 * errs['plain'][1], errs
